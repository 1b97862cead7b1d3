// The principal basis of the reject filter's 64-byte rows, alone (instant-distance_amd/csrc/idist_basis.hpp: host code, no HIP).
// Whatever the sample — low-rank, constant, fewer rows than directions, non-finite entries — B must come out orthonormal after its
// rounding to f32 (|B B^T - I|_inf <= 1e-6), s >= 1 must bound its largest singular value, and two calls must agree bit for bit.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../instant-distance_amd/csrc/idist_basis.hpp"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform() {                      // xorshift64*, in (0, 1)
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return ((rng_state * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0) + 1e-17;
}
static double normal() { return std::sqrt(-2.0 * std::log(uniform())) * std::cos(6.283185307179586 * uniform()); }

static int check(const char* name, const std::vector<float>& x, uint32_t ns, uint32_t d, bool want_spread) {
    const idist::PrincipalBasis a = idist::principal_basis(x.data(), ns, d, d);
    const idist::PrincipalBasis b = idist::principal_basis(x.data(), ns, d, d);
    const int m = idist::kBasisM;
    int bad = 0;
    if (a.B.size() != (size_t)m * d || a.mu.size() != d) { printf("%s: sizes\n", name); return 1; }
    if (memcmp(a.B.data(), b.B.data(), a.B.size() * 4) || memcmp(a.mu.data(), b.mu.data(), d * 4) || a.s != b.s) { printf("%s: two calls differ\n", name); bad++; }
    double worst = 0.0, sig2 = 0.0;
    for (int i = 0; i < m; i++) {
        double row = 0.0, rs = 0.0;
        for (int j = 0; j < m; j++) {
            double dot = 0.0;
            for (uint32_t k = 0; k < d; k++) dot += (double)a.B[(size_t)i * d + k] * (double)a.B[(size_t)j * d + k];
            row += std::fabs(dot - (i == j ? 1.0 : 0.0));
            rs += std::fabs(dot);
        }
        worst = std::max(worst, row);
        sig2 = std::max(sig2, rs);
    }
    if (!(worst <= 1e-6)) { printf("%s: |B B^T - I|_inf = %g\n", name, worst); bad++; }
    if (!(a.s >= 1.0) || !(a.s * a.s >= sig2) || !(a.s < 1.001)) { printf("%s: s = %.17g, |B B^T|_inf = %.17g\n", name, a.s, sig2); bad++; }
    for (uint32_t k = 0; k < d; k++)
        if (!std::isfinite(a.mu[k])) { printf("%s: mu[%u] is not finite\n", name, k); bad++; break; }
    if (want_spread) {
        // the directions come in order of falling variance and the first ones hold what there is: 8 latent dimensions -> the 8 leading
        // directions carry (almost) all of the centred sample's energy
        double total = 0.0, lead8 = 0.0, prev = std::numeric_limits<double>::infinity();
        std::vector<double> var(m, 0.0);
        for (uint32_t r = 0; r < ns; r++) {
            for (uint32_t k = 0; k < d; k++) { const double c = (double)x[(size_t)r * d + k] - (double)a.mu[k]; total += c * c; }
            for (int i = 0; i < m; i++) {
                double y = 0.0;
                for (uint32_t k = 0; k < d; k++) y += (double)a.B[(size_t)i * d + k] * ((double)x[(size_t)r * d + k] - (double)a.mu[k]);
                var[i] += y * y;
            }
        }
        for (int i = 0; i < m; i++) {
            if (i < 8) lead8 += var[i];
            if (var[i] > prev * (1.0 + 1e-6) + 1e-12 * total) { printf("%s: variance rises at direction %d\n", name, i); bad++; break; }
            prev = var[i];
        }
        if (!(lead8 >= 0.9 * total)) { printf("%s: 8 leading directions hold %.3f of the energy\n", name, lead8 / total); bad++; }
    }
    printf("%s: |B B^T - I|_inf = %.3g, s - 1 = %.3g\n", name, worst, a.s - 1.0);
    return bad;
}

int main() {
    int bad = 0;
    {   // 2048 x 300, 8 latent dimensions + a little noise, off the origin
        const uint32_t ns = 2048, d = 300, lat = 8;
        std::vector<double> A((size_t)lat * d);
        for (double& v : A) v = normal();
        std::vector<float> x((size_t)ns * d);
        for (uint32_t r = 0; r < ns; r++) {
            double z[lat];
            for (uint32_t l = 0; l < lat; l++) z[l] = normal();
            for (uint32_t k = 0; k < d; k++) {
                double v = 0.02 * normal() + 3.0;
                for (uint32_t l = 0; l < lat; l++) v += z[l] * A[(size_t)l * d + k];
                x[(size_t)r * d + k] = (float)v;
            }
        }
        bad += check("lowrank 2048 x 300", x, ns, d, true);
        x[5 * d + 7] = std::numeric_limits<float>::quiet_NaN();
        x[9 * d + 0] = std::numeric_limits<float>::infinity();
        x[11 * d + 299] = -std::numeric_limits<float>::infinity();
        bad += check("the same with non-finite entries", x, ns, d, false);
    }
    {
        std::vector<float> x((size_t)2048 * 300, 0.5f);
        bad += check("constant 2048 x 300", x, 2048, 300, false);
    }
    {   // fewer rows than directions
        const uint32_t ns = 20, d = 300;
        std::vector<float> x((size_t)ns * d);
        for (float& v : x) v = (float)uniform();
        bad += check("20 x 300", x, ns, d, false);
    }
    {   // extreme scales
        std::vector<float> x((size_t)256 * 128);
        for (float& v : x) v = (float)(normal() * 1e30);
        bad += check("256 x 128 at 1e30", x, 256, 128, false);
        for (float& v : x) v = (float)(normal() * 1e-30);
        bad += check("256 x 128 at 1e-30", x, 256, 128, false);
    }
    if (bad) { printf("%d failures\n", bad); return 1; }
    printf("basis ok\n");
    return 0;
}
