// idist_kmeans.hpp — Lloyd's k-means for at most 64 clusters: what cuts the points of a partitioned index into parts whose
// centroids can route a query (idist_route.hpp).  include/idist.h has the definitions; in short
//
//   assign   a(i) = arg min_j d~(x_i, c_j),  d~ = |x|^2 + |c|^2 - 2 x.c in f32 (the product form of idist_mfma.hpp), a strict `<` scan
//            from j = 0; a row whose computed |x|^2 is not finite gets i mod k;
//   update   c_j = (sum of the member rows) / count_j, the sum formed chunk by chunk of `chunk` rows in row order and the chunks
//            added in chunk order: no float atomics, the same bytes whatever the grid.
//
// kmeans_assign_kernel is the hot one — every row against every centroid, once per iteration — and a dense contraction, so it runs on
// the f32 matrix cores.  A workgroup of four waves owns 128 rows, a wave 32 of them against all 64 centroid columns:
//
//   * v_mfma_f32_32x32x2_f32 with the CENTROIDS as the A operand and the data rows as B.  The C/D layout puts column j = lane & 31 in
//     a lane, so with the rows as columns each of the two 32 x 32 accumulators holds, per lane, 16 centroids of ONE row: the arg-min
//     over 64 centroids is 32 comparisons in registers and one exchange with lane ^ 32 — no LDS, no transposition.  Register order is
//     not centroid order across the two halves of the wave (rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5)), so the exchange compares
//     (d~, j) pairs and the smaller j wins a tie explicitly.
//   * K is consumed in chunks of 32 floats staged in LDS at the 36-float pitch of idist_mfma.hpp (16-byte rows, 36 = 4 * 9: the
//     ds_read_b128 of 16 lanes on rows that differ mod 16 touch 64 distinct banks); the next chunk is requested global -> registers
//     before the current one's MFMAs.  Instruction q of a chunk contracts elements q (lanes 0-31) and 16 + q (lanes 32-63), so a
//     lane's sixteen operands are contiguous in its row.
//   * the centroid matrix is staged ONCE per workgroup, [64][Kp + 4] floats (Kp = dim rounded up to the chunk; Kp + 4 is again
//     4 * odd), while it fits the 64 KiB a workgroup gets without opting in to more beside the row tile — dim <= 160; longer rows
//     stage the centroids' chunk next to the rows' (9 KiB per chunk from L2 beside 18 KiB from HBM), which keeps five workgroups
//     on a CU where the whole 300-d matrix (83 KiB) would leave one wave per SIMD to hide the HBM latency.
//   * |x|^2 is accumulated from the B operands of the same pass (one chain per half of the wave, added once): a row is read from
//     HBM exactly once per assign.  The centroids' norms come from kmeans_prep_kernel, +inf for the padded columns j >= k; K is
//     padded with zeros, rows past n are staged as zeros and never written.
//   * with k <= 32 the second accumulator is skipped (its columns are all padding): half the matrix work.
#pragma once
#include "idist_mfma.hpp"

namespace idist {

constexpr int kKmRows = 128, kKmCols = 64, kKmKC = 32, kKmPitch = 36;
constexpr uint32_t kKmLdsBudget = 64 * 1024;
constexpr uint32_t kKmHeadFloats = kKmRows * kKmPitch + 2 * kKmCols;          // row tile, |c|^2, the workgroup's histogram

__host__ __device__ inline uint32_t km_kpad(uint32_t dim) { return (dim + (uint32_t)kKmKC - 1u) & ~((uint32_t)kKmKC - 1u); }
__host__ __device__ inline bool km_resident(uint32_t dim) { return ((size_t)kKmHeadFloats + (size_t)kKmCols * (km_kpad(dim) + 4u)) * 4u <= kKmLdsBudget; }
__host__ __device__ inline size_t km_assign_smem(uint32_t dim) {
    return ((size_t)kKmHeadFloats + (size_t)kKmCols * (km_resident(dim) ? km_kpad(dim) + 4u : (uint32_t)kKmPitch)) * 4u;
}
__device__ __forceinline__ bool km_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// |c_j|^2 for j < k (a k-ordered fma chain per lane), +inf for the padded columns; clears what the assign kernel adds to
__global__ __launch_bounds__(64) void kmeans_prep_kernel(const float* __restrict__ cent, uint32_t k, uint32_t dim, float* __restrict__ cn,
                                                        uint32_t* counts, uint32_t* changed) {
    const uint32_t j = threadIdx.x;
    float acc = __uint_as_float(0x7f800000u);
    if (j < k) {
        acc = 0.0f;
        for (uint32_t e = 0; e < dim; e++) acc = __builtin_fmaf(cent[(size_t)j * dim + e], cent[(size_t)j * dim + e], acc);
        if (counts) counts[j] = 0u;
    }
    cn[j] = acc;
    if (j == 0 && changed) *changed = 0u;
}

struct KmAssignArgs {
    const float* X;            // [n][dim] natural rows
    const float* C;            // [k][dim]
    const float* cn;           // [64] from kmeans_prep_kernel
    uint32_t n, dim, k;
    uint32_t vec4;             // dim % 4 == 0 and both matrices 16-byte aligned: 16-byte global loads
    uint32_t* assign;          // [n]
    const uint32_t* prev;      // [n] or nullptr: *changed |= 1 when a row's cluster differs
    uint32_t* changed;
    uint32_t* counts;          // [k] or nullptr (cleared by kmeans_prep_kernel)
    uint32_t* bad;             // [n] or nullptr: 1 for a row whose |x|^2 is not finite
};

// four floats of row `row` (of `rows`) from column `col`, zeros past the row and past the matrix
__device__ __forceinline__ float4 km_load4(const float* __restrict__ M, uint32_t rows, uint32_t dim, uint32_t row, uint32_t col, bool vec4) {
    float4 v;
    v.x = v.y = v.z = v.w = 0.0f;
    if (row >= rows || col >= dim) return v;
    const float* p = M + (size_t)row * dim + col;
    if (vec4) return *reinterpret_cast<const float4*>(p);
    v.x = p[0];
    if (col + 1u < dim) v.y = p[1];
    if (col + 2u < dim) v.z = p[2];
    if (col + 3u < dim) v.w = p[3];
    return v;
}

__global__ __launch_bounds__(256) void kmeans_assign_kernel(KmAssignArgs a) {
    IDIST_DYN_SMEM(smem_raw);
    float* Xs = reinterpret_cast<float*>(smem_raw);                       // [128][36] one K chunk of the row tile
    float* cn_s = Xs + kKmRows * kKmPitch;                                // [64]
    uint32_t* hist = reinterpret_cast<uint32_t*>(cn_s + kKmCols);         // [64]
    float* Cs = reinterpret_cast<float*>(hist + kKmCols);                 // resident: [64][Kp + 4]; else [64][36], one K chunk
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6, half = lane >> 5;
    const uint32_t Kp = km_kpad(a.dim), kf4 = Kp / 4u;
    const bool resident = km_resident(a.dim), two = a.k > 32u, vec4 = a.vec4 != 0u;
    const uint32_t cpitch = resident ? Kp + 4u : (uint32_t)kKmPitch;
    if (tid < kKmCols) { cn_s[tid] = a.cn[tid]; hist[tid] = 0u; }
    if (resident)
        for (uint32_t idx = (uint32_t)tid; idx < (uint32_t)kKmCols * kf4; idx += 256u) {
            const uint32_t row = idx / kf4, part = (idx % kf4) << 2;
            *reinterpret_cast<float4*>(Cs + row * cpitch + part) = km_load4(a.C, a.k, a.dim, row, part, vec4);
        }
    block_sync();
    const uint32_t ntiles = (a.n + (uint32_t)kKmRows - 1u) / (uint32_t)kKmRows;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t r0 = tile * (uint32_t)kKmRows;
        f32x16 acc0, acc1;
        for (int r = 0; r < 16; r++) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
        float xn = 0.0f;
        // 1024 float4 of rows (4 per thread) and, when the centroids are staged per chunk, 512 of theirs (2 per thread)
        auto fetch = [&](uint32_t kc, float4 (&vx)[4], float4 (&vc)[2]) {
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t idx = (uint32_t)tid + 256u * (uint32_t)u;
                vx[u] = km_load4(a.X, a.n, a.dim, r0 + (idx >> 3), kc + ((idx & 7u) << 2), vec4);
            }
            if (!resident) {
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    const uint32_t idx = (uint32_t)tid + 256u * (uint32_t)u;
                    vc[u] = km_load4(a.C, a.k, a.dim, idx >> 3, kc + ((idx & 7u) << 2), vec4);
                }
            }
        };
        float4 px[4], pc[2];
        fetch(0u, px, pc);
        for (uint32_t kc = 0; kc < Kp; kc += (uint32_t)kKmKC) {
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int idx = tid + 256 * u;
                *reinterpret_cast<float4*>(Xs + (idx >> 3) * kKmPitch + ((idx & 7) << 2)) = px[u];
            }
            if (!resident) {
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    const int idx = tid + 256 * u;
                    *reinterpret_cast<float4*>(Cs + (idx >> 3) * kKmPitch + ((idx & 7) << 2)) = pc[u];
                }
            }
            block_sync();
            if (kc + (uint32_t)kKmKC < Kp) fetch(kc + (uint32_t)kKmKC, px, pc);
            const float* bp = Xs + (w * 32 + (lane & 31)) * kKmPitch + 16 * half;
            const float* ap = Cs + (uint32_t)(lane & 31) * cpitch + (resident ? kc : 0u) + 16u * (uint32_t)half;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float4 b = *reinterpret_cast<const float4*>(bp + 4 * q);
                const float4 a0 = *reinterpret_cast<const float4*>(ap + 4 * q);
                xn = __builtin_fmaf(b.x, b.x, xn);
                xn = __builtin_fmaf(b.y, b.y, xn);
                xn = __builtin_fmaf(b.z, b.z, xn);
                xn = __builtin_fmaf(b.w, b.w, xn);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b.x, acc0, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b.y, acc0, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, b.z, acc0, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, b.w, acc0, 0, 0, 0);
                if (two) {
                    const float4 a1 = *reinterpret_cast<const float4*>(ap + 32u * cpitch + 4 * q);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b.x, acc1, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b.y, acc1, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, b.z, acc1, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, b.w, acc1, 0, 0, 0);
                }
            }
            block_sync();
        }
        // ---- the row's arg-min.  The strict `<` scan from j = 0 keeps a NaN at j = 0 for good and never takes a later one: a NaN
        //      is -inf at j = 0 and +inf elsewhere, and the order is (d~, j).  A lane's registers ARE in ascending j.
        xn += __shfl_xor(xn, 32, 64);                                    // (the same bits in both halves: one addition, commutative)
        float bd = 0.0f;
        uint32_t bj = 0u;
#pragma unroll
        for (int t = 0; t < 2; t++) {
            if (t == 1 && !two) break;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const uint32_t j = 32u * (uint32_t)t + (uint32_t)((r & 3) + 8 * (r >> 2) + 4 * half);
                float d = (xn + cn_s[j]) - 2.0f * (t ? acc1[r] : acc0[r]);
                if (d != d) d = __uint_as_float(j == 0u ? 0xff800000u : 0x7f800000u);
                if ((t == 0 && r == 0) || d < bd) { bd = d; bj = j; }
            }
        }
        const float od = __shfl_xor(bd, 32, 64);
        const uint32_t oj = (uint32_t)__shfl_xor((int)bj, 32, 64);
        if (od < bd || (od == bd && oj < bj)) bj = oj;
        const uint32_t row = r0 + (uint32_t)(w * 32 + (lane & 31));
        if (half == 0 && row < a.n) {
            const bool fin = km_finite(xn);
            const uint32_t c = fin ? bj : row % a.k;
            a.assign[row] = c;
            if (a.bad) a.bad[row] = fin ? 0u : 1u;
            if (a.prev && a.prev[row] != c) atomicOr(a.changed, 1u);
            if (a.counts) atomicAdd(&hist[c], 1u);
        }
    }
    block_sync();
    if (a.counts && (uint32_t)tid < a.k && hist[tid]) atomicAdd(&a.counts[tid], hist[tid]);
}

// bad[i] = 1 where the |x_i|^2 kmeans_assign_kernel computes is not finite — the same two chains in the same order (elements
// kc + 16 h .. kc + 16 h + 15 of every chunk kc go to chain h; the padding adds exact zeros) — for an update that is handed an
// assignment from outside.  Two lanes per row.
__global__ __launch_bounds__(64) void kmeans_rowflags_kernel(const float* __restrict__ X, uint32_t n, uint32_t dim, uint32_t* __restrict__ bad) {
    const uint32_t lane = threadIdx.x, h = lane & 1u;
    for (uint32_t base = blockIdx.x * 32u; base < n; base += gridDim.x * 32u) {      // (uniform: the exchange below is a wave's)
        const uint32_t row = base + (lane >> 1);
        float acc = 0.0f;
        if (row < n)
            for (uint32_t kc = 16u * h; kc < dim; kc += (uint32_t)kKmKC)
                for (uint32_t e = kc; e < kc + 16u && e < dim; e++) acc = __builtin_fmaf(X[(size_t)row * dim + e], X[(size_t)row * dim + e], acc);
        const float other = __shfl_xor(acc, 1, 64);
        if (row < n && h == 0u) bad[row] = km_finite(acc + other) ? 0u : 1u;
    }
}

struct KmUpdateArgs {
    const float* X;            // [n][dim]
    const uint32_t* assign;    // [n], every value < k
    const uint32_t* bad;       // [n]
    uint32_t n, dim, k, chunk;
    float* part;               // [n_chunks][k][dim] the chunks' sums
    uint32_t* cpart;           // [n_chunks][k][2]   the chunks' members and summed members
};

// One single-wave workgroup per (row chunk, tile of 64 columns): lane l owns column l of the LDS table [k][64] and adds the chunk's
// rows into it in row order — one owner per cell, so the order of every sum is the rows'.  Lane 0 of the first column tile counts.
__global__ __launch_bounds__(64) void kmeans_partial_kernel(KmUpdateArgs a) {
    IDIST_DYN_SMEM(smem_raw);
    float* tab = reinterpret_cast<float*>(smem_raw);                      // [k][64]
    uint32_t* cnt = reinterpret_cast<uint32_t*>(tab + a.k * 64u);         // [k][2]
    const uint32_t lane = threadIdx.x;
    const uint32_t nct = (a.dim + 63u) / 64u, nch = (a.n + a.chunk - 1u) / a.chunk;
    for (uint32_t item = blockIdx.x; item < nch * nct; item += gridDim.x) {
        const uint32_t ch = item / nct, ct = item - ch * nct, col = ct * 64u + lane;
        for (uint32_t j = 0; j < a.k; j++) tab[j * 64u + lane] = 0.0f;
        if (lane < a.k) { cnt[2u * lane] = 0u; cnt[2u * lane + 1u] = 0u; }
        wave_sync();
        const uint32_t lo = ch * a.chunk, hi = a.n - lo < a.chunk ? a.n : lo + a.chunk;
#pragma unroll 4
        for (uint32_t r = lo; r < hi; r++) {
            const uint32_t j = a.assign[r], b = a.bad[r];
            if (j >= a.k) continue;
            if (ct == 0u && lane == 0u) { cnt[2u * j]++; if (!b) cnt[2u * j + 1u]++; }
            if (!b && col < a.dim) tab[j * 64u + lane] += a.X[(size_t)r * a.dim + col];
        }
        wave_sync();
        if (col < a.dim)
            for (uint32_t j = 0; j < a.k; j++) a.part[((size_t)ch * a.k + j) * a.dim + col] = tab[j * 64u + lane];
        if (ct == 0u && lane < a.k) {
            a.cpart[((size_t)ch * a.k + lane) * 2u] = cnt[2u * lane];
            a.cpart[((size_t)ch * a.k + lane) * 2u + 1u] = cnt[2u * lane + 1u];
        }
        wave_sync();
    }
}

// c_j = (the chunks' sums added in chunk order) / (summed members), one division per coordinate; a cluster without summed members
// keeps its centroid.  counts[j] = members.
__global__ __launch_bounds__(256) void kmeans_reduce_kernel(const float* __restrict__ part, const uint32_t* __restrict__ cpart, uint32_t nch,
                                                           uint32_t k, uint32_t dim, float* __restrict__ cent, uint32_t* __restrict__ counts) {
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < k * dim; idx += gridDim.x * 256u) {
        const uint32_t j = idx / dim, col = idx - j * dim;
        uint32_t members = 0u, summed = 0u;
        float s = 0.0f;
        for (uint32_t ch = 0; ch < nch; ch++) {
            members += cpart[((size_t)ch * k + j) * 2u];
            summed += cpart[((size_t)ch * k + j) * 2u + 1u];
            s += part[((size_t)ch * k + j) * dim + col];
        }
        if (summed) cent[idx] = s / (float)summed;
        if (col == 0u) counts[j] = members;
    }
}

}  // namespace idist
