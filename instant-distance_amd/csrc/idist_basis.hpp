// The principal basis of the reject filter's 64-byte rows: host code only, f64, deterministic — a pure function of
// the sample it is given, so that replicas and re-imports of an index arrive at the same basis (and the same format policy).
//
// principal_basis() returns m = kBasisM orthonormal directions of largest sample variance, B [m][d], rounded to f32, and the sample
// mean mu [d] (f32, from the finite values of each coordinate), for a sample of ns rows of d coordinates.  Only ORTHONORMALITY bears on
// correctness — the filter's bound reads |B x| <= s |x| with s >= sigma_max(B_f32), returned beside B — the quality of the directions
// decides how many candidates the bound rejects, never a result.  Degenerate samples (constant data, fewer independent rows than m,
// non-finite entries) still give an orthonormal B: Gram-Schmidt completes it with unit vectors.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace idist {

constexpr int kBasisM = 56;          // coordinates of a principal row: 56 one-byte codes + 8 bytes of metadata = one 64-B request

struct PrincipalBasis {
    std::vector<float> B;            // [kBasisM][d], rows orthonormal up to f32 rounding, in order of falling sample variance
    std::vector<float> mu;           // [d]
    double s = 1.0;                  // >= max(1, sigma_max(B as stored in f32)): sqrt(|B B^T|_inf), rounded up
};

namespace basis_detail {
// Modified Gram-Schmidt, every column against its predecessors TWICE; a column that has (numerically) nothing of its own left is
// replaced by the first unit vector that has — V [m][d] (row j = vector j) ends up orthonormal whatever it held.
inline void orthonormalize(std::vector<double>& V, int m, uint32_t d) {
    uint32_t next_unit = 0;
    for (int j = 0; j < m; j++) {
        double* v = &V[(size_t)j * d];
        for (;;) {
            double n0 = 0.0;
            for (uint32_t k = 0; k < d; k++) n0 += v[k] * v[k];
            for (int pass = 0; pass < 2; pass++)
                for (int i = 0; i < j; i++) {
                    const double* u = &V[(size_t)i * d];
                    double dot = 0.0;
                    for (uint32_t k = 0; k < d; k++) dot += u[k] * v[k];
                    for (uint32_t k = 0; k < d; k++) v[k] -= dot * u[k];
                }
            double n1 = 0.0;
            for (uint32_t k = 0; k < d; k++) n1 += v[k] * v[k];
            if (std::isfinite(n0) && std::isfinite(n1) && n1 > 0.0 && n1 >= 1e-20 * n0 && n1 > 1e-280) {
                const double inv = 1.0 / std::sqrt(n1);
                for (uint32_t k = 0; k < d; k++) v[k] *= inv;
                break;
            }
            // (a unit vector loses at most everything it shares with j < d earlier vectors: among any j + 1 of them one keeps >= 1 / (j + 1))
            for (uint32_t k = 0; k < d; k++) v[k] = 0.0;
            v[next_unit % d] = 1.0;
            next_unit++;
        }
    }
}
// cyclic Jacobi on the symmetric H [m][m]: H -> diagonal, Z [m][m] (column c = eigenvector c) accumulates the rotations
inline void jacobi(std::vector<double>& H, std::vector<double>& Z, int m) {
    for (int i = 0; i < m; i++)
        for (int j = 0; j < m; j++) Z[(size_t)i * m + j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; sweep++) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < m; i++)
            for (int j = 0; j < m; j++) (i == j ? diag : off) += H[(size_t)i * m + j] * H[(size_t)i * m + j];
        if (!(off > 1e-30 * diag)) break;
        for (int p = 0; p < m - 1; p++)
            for (int q = p + 1; q < m; q++) {
                const double apq = H[(size_t)p * m + q];
                if (apq == 0.0) continue;
                const double theta = (H[(size_t)q * m + q] - H[(size_t)p * m + p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < m; k++) {
                    const double hkp = H[(size_t)k * m + p], hkq = H[(size_t)k * m + q];
                    H[(size_t)k * m + p] = c * hkp - s * hkq;
                    H[(size_t)k * m + q] = s * hkp + c * hkq;
                }
                for (int k = 0; k < m; k++) {
                    const double hpk = H[(size_t)p * m + k], hqk = H[(size_t)q * m + k];
                    H[(size_t)p * m + k] = c * hpk - s * hqk;
                    H[(size_t)q * m + k] = s * hpk + c * hqk;
                }
                for (int k = 0; k < m; k++) {
                    const double zkp = Z[(size_t)k * m + p], zkq = Z[(size_t)k * m + q];
                    Z[(size_t)k * m + p] = c * zkp - s * zkq;
                    Z[(size_t)k * m + q] = s * zkp + c * zkq;
                }
            }
    }
}
}  // namespace basis_detail

// x: [ns][ld] f32, the first d entries of a row are its coordinates.  d >= kBasisM.
inline PrincipalBasis principal_basis(const float* x, uint32_t ns, uint32_t d, size_t ld) {
    using namespace basis_detail;
    constexpr int m = kBasisM;
    PrincipalBasis out;
    out.mu.assign(d, 0.0f);
    out.B.assign((size_t)m * d, 0.0f);
    // the mean of every coordinate's finite values
    {
        std::vector<double> sum(d, 0.0);
        std::vector<uint32_t> cnt(d, 0u);
        for (uint32_t r = 0; r < ns; r++)
            for (uint32_t k = 0; k < d; k++) {
                const float v = x[(size_t)r * ld + k];
                if (std::fabs(v) <= 3.0e38f) { sum[k] += v; cnt[k]++; }
            }
        for (uint32_t k = 0; k < d; k++) out.mu[k] = cnt[k] ? (float)(sum[k] / cnt[k]) : 0.0f;
    }
    // covariance of the centred sample (non-finite entries count as the mean), scaled to O(1) so that nothing under- or overflows
    std::vector<double> X((size_t)ns * d);
    double amax = 0.0;
    for (uint32_t r = 0; r < ns; r++)
        for (uint32_t k = 0; k < d; k++) {
            const float v = x[(size_t)r * ld + k];
            const double c = std::fabs(v) <= 3.0e38f ? (double)v - (double)out.mu[k] : 0.0;
            X[(size_t)r * d + k] = c;
            amax = std::max(amax, std::fabs(c));
        }
    if (amax > 0.0) {
        const double inv = 1.0 / amax;
        for (double& v : X) v *= inv;
    }
    std::vector<double> C((size_t)d * d, 0.0);
    for (uint32_t r = 0; r < ns; r++) {
        const double* xr = &X[(size_t)r * d];
        for (uint32_t i = 0; i < d; i++) {
            const double xi = xr[i];
            if (xi == 0.0) continue;
            double* ci = &C[(size_t)i * d];
            for (uint32_t j = i; j < d; j++) ci[j] += xi * xr[j];
        }
    }
    for (uint32_t i = 0; i < d; i++)
        for (uint32_t j = 0; j < i; j++) C[(size_t)i * d + j] = C[(size_t)j * d + i];
    // block power iteration from the m coordinates of largest variance (ties: the lower index)
    std::vector<uint32_t> order(d);
    for (uint32_t k = 0; k < d; k++) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return C[(size_t)a * d + a] > C[(size_t)b * d + b]; });
    std::vector<double> V((size_t)m * d, 0.0), W((size_t)m * d);
    for (int j = 0; j < m; j++) V[(size_t)j * d + order[j]] = 1.0;
    auto times_C = [&](const std::vector<double>& in, std::vector<double>& res) {
        for (int j = 0; j < m; j++) {
            double* w = &res[(size_t)j * d];
            for (uint32_t k = 0; k < d; k++) w[k] = 0.0;
            const double* v = &in[(size_t)j * d];
            for (uint32_t i = 0; i < d; i++) {
                const double vi = v[i];
                if (vi == 0.0) continue;
                const double* ci = &C[(size_t)i * d];
                for (uint32_t k = 0; k < d; k++) w[k] += vi * ci[k];
            }
        }
    };
    for (int it = 0; it < 12; it++) {
        times_C(V, W);
        // (a direction C annihilates keeps what it was: the null space of a degenerate sample must not turn into zeros)
        for (int j = 0; j < m; j++) {
            double n = 0.0;
            for (uint32_t k = 0; k < d; k++) n += W[(size_t)j * d + k] * W[(size_t)j * d + k];
            if (!(n > 0.0) || !std::isfinite(n)) std::copy(&V[(size_t)j * d], &V[(size_t)j * d] + d, &W[(size_t)j * d]);
        }
        V.swap(W);
        orthonormalize(V, m, d);
    }
    // Rayleigh-Ritz inside the subspace: the directions in order of falling variance (the lattice's range comes from the first)
    times_C(V, W);
    std::vector<double> H((size_t)m * m), Z((size_t)m * m);
    for (int i = 0; i < m; i++)
        for (int j = 0; j < m; j++) {
            double dot = 0.0;
            for (uint32_t k = 0; k < d; k++) dot += V[(size_t)i * d + k] * W[(size_t)j * d + k];
            H[(size_t)i * m + j] = dot;
        }
    for (int i = 0; i < m; i++)
        for (int j = 0; j < i; j++) H[(size_t)i * m + j] = H[(size_t)j * m + i] = 0.5 * (H[(size_t)i * m + j] + H[(size_t)j * m + i]);
    jacobi(H, Z, m);
    std::vector<int> eo(m);
    for (int i = 0; i < m; i++) eo[i] = i;
    std::stable_sort(eo.begin(), eo.end(), [&](int a, int b) { return H[(size_t)a * m + a] > H[(size_t)b * m + b]; });
    for (int j = 0; j < m; j++) {
        double* w = &W[(size_t)j * d];
        for (uint32_t k = 0; k < d; k++) w[k] = 0.0;
        for (int i = 0; i < m; i++) {
            const double z = Z[(size_t)i * m + eo[j]];
            const double* v = &V[(size_t)i * d];
            for (uint32_t k = 0; k < d; k++) w[k] += z * v[k];
        }
    }
    orthonormalize(W, m, d);
    for (size_t i = 0; i < (size_t)m * d; i++) out.B[i] = (float)W[i];
    // s >= sigma_max(B_f32): sigma_max^2 = |B B^T|_2 <= |B B^T|_inf, evaluated in f64 (the products of f32 values are exact there)
    double norm = 0.0;
    for (int i = 0; i < m; i++) {
        double row = 0.0;
        for (int j = 0; j < m; j++) {
            double dot = 0.0;
            for (uint32_t k = 0; k < d; k++) dot += (double)out.B[(size_t)i * d + k] * (double)out.B[(size_t)j * d + k];
            row += std::fabs(dot);
        }
        norm = std::max(norm, row);
    }
    out.s = std::max(1.0, std::sqrt(norm) * (1.0 + 1e-9));
    return out;
}

}  // namespace idist
