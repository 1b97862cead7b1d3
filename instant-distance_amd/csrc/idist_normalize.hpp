// idist_normalize.hpp — the two passes behind IDIST_METRIC_COSINE (include/idist.h): a cosine index IS the squared-L2 index over the
// normalised rows x^ = x / sqrt(s(x)), and the distance it reports is half the canonical squared-L2 distance of two normalised
// vectors (|q^ - x^|^2 / 2 = 1 - cos).  The search, build and brute-force kernels never learn about it: they keep seeing metric 0.
//
// normalize_rows_kernel: s(x) is the canonical Point::distance(x, origin) — the SAME fold every distance of this engine uses
// (py/lib.rs:378-421: eight fused-multiply-add chains over chunks of eight, lo + hi halves, the 4-wide tail, (s0+s2)+(s1+s3)), so
// its bits are the oracle's.  A chain is a sequential dependency: eight lanes (one per chain) are all a row can use, so a wave
// takes EIGHT rows at a time, group g = lane >> 3 one row, lane j = lane & 7 chain j — the assignment of dist_rounds
// (idist_device.hpp), with fold_chains as its fold.  Two layouts, one code path:
//   * the index's blocked rows (nb full 32-float blocks: lane j's 16 bytes at 32 t + 4 j ARE chain j's steps 4 t .. 4 t + 3; the
//     remaining steps and the tail follow in natural order) — 16-byte loads throughout;
//   * natural [n][dim] rows (queries, the standalone entry) are the same thing with nb = 0: chain j reads element 8 s + j of step s,
//     4 bytes per lane and 32 contiguous bytes per row and step (elements beyond dim count as 0: fma(0, 0, acc) == acc).
// r = sqrt(s) and x / r are correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt).  A row whose r is not a positive finite
// number — zero rows, NaN / inf coordinates, an s that overflowed or underflowed — is copied unchanged.  The second pass re-reads
// the row (just read: L2) and divides, 16 bytes per lane where row length and both pointers allow, so `out` may be `in` itself
// (every element is read and written by the same lane, after the row's sum is complete).  Grid-stride over groups of 8 rows, no
// atomics, no LDS.
//
// scale_half_kernel: d -> 0.5f * d over the [nq][ef] distances of a launch (one f32 multiply: exact unless d is denormal; +inf
// padding stays +inf, the engine's one NaN pattern stays as it is).
#pragma once
#include "idist_device.hpp"

namespace idist {

// s(x) of one row for the eight lanes of a group (lane j = lane & 7 runs chain j): `src` holds `dim` coordinates in the layout (nb
// full blocks, natural remainder; natural rows: nb = 0).  `on` false: the group has no row (the lanes still take part in the
// fold's cross-lane moves).  The result is valid in all eight lanes.  Shared by the cosine and the inner-product passes
// (idist_dot.hpp): ONE statement of the fold.
__device__ __forceinline__ float row_norm2_group(const float* src, bool on, uint32_t dim, uint32_t nb, int lane) {
    const int j = lane & 7;
    const uint32_t dp = (dim + 3u) & ~3u, steps = dp / 8u, rs = steps - 4u * nb;   // chain steps beyond the blocks
    const bool tail = (dp % 8u) == 4u;
    const uint32_t rem0 = 32u * nb, tail0 = rem0 + 8u * rs + (uint32_t)(j & 3);
    float acc = 0.0f;
    if (on) {
        for (uint32_t t = 0; t < nb; t++) {
            const float4 v = *reinterpret_cast<const float4*>(src + 32u * t + 4u * (uint32_t)j);
            acc = __builtin_fmaf(v.x, v.x, acc);
            acc = __builtin_fmaf(v.y, v.y, acc);
            acc = __builtin_fmaf(v.z, v.z, acc);
            acc = __builtin_fmaf(v.w, v.w, acc);
        }
        for (uint32_t s = 0; s < rs; s++) {
            const uint32_t e = rem0 + 8u * s + (uint32_t)j;      // (natural there: position == element)
            const float x = e < dim ? src[e] : 0.0f;
            acc = __builtin_fmaf(x, x, acc);
        }
    }
    const float tq = on && tail && tail0 < dim ? src[tail0] : 0.0f;
    const float s = fold_chains(acc, tail, tq, 0.0f);            // valid in lane j == 0 of the group
    return __uint_as_float(bcast_u32(__float_as_uint(s), lane & ~7));
}

// rows: [n][ld] floats holding `dim` coordinates each in the layout (nb, natural remainder); vec != 0: ld % 4 == 0 and both
// pointers 16-byte aligned.  out_norm2 (may be nullptr): s(x) per row.
__global__ __launch_bounds__(64) void normalize_rows_kernel(const float* in, float* out, uint32_t n, uint32_t dim, uint32_t ld,
                                                            uint32_t nb, uint32_t vec, float* out_norm2) {
    const int lane = lane_id(), g = lane >> 3, j = lane & 7;
    const uint32_t groups = (n + 7u) / 8u;
    for (uint32_t b = blockIdx.x; b < groups; b += gridDim.x) {
        const uint32_t row = 8u * b + (uint32_t)g;
        const bool on = row < n;
        const float* src = in + (size_t)(on ? row : 0u) * ld;
        const float s0 = row_norm2_group(src, on, dim, nb, lane);
        const float r = __builtin_sqrtf(s0);
        const bool scale = r > 0.0f && r < __builtin_inff();         // (NaN fails both)
        if (!on) continue;
        if (out_norm2 && j == 0) out_norm2[row] = s0;
        float* dst = out + (size_t)row * ld;
        if (vec) {
            for (uint32_t f = (uint32_t)j; f < ld / 4u; f += 8u) {
                float4 v = *reinterpret_cast<const float4*>(src + 4u * f);
                if (scale) { v.x = v.x / r; v.y = v.y / r; v.z = v.z / r; v.w = v.w / r; }
                *reinterpret_cast<float4*>(dst + 4u * f) = v;
            }
        } else {
            for (uint32_t e = (uint32_t)j; e < ld; e += 8u) {
                const float x = src[e];
                dst[e] = scale ? x / r : x;
            }
        }
    }
}

__global__ void scale_half_kernel(float* d, size_t total, uint32_t vec) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
    auto half = [](float x) { return x != x ? x : 0.5f * x; };
    const size_t n4 = vec ? total / 4u : 0u;
    for (size_t f = tid; f < n4; f += nth) {
        float4 v = *reinterpret_cast<const float4*>(d + 4u * f);
        v.x = half(v.x); v.y = half(v.y); v.z = half(v.z); v.w = half(v.w);
        *reinterpret_cast<float4*>(d + 4u * f) = v;
    }
    for (size_t i = 4u * n4 + tid; i < total; i += nth) d[i] = half(d[i]);
}

}  // namespace idist
