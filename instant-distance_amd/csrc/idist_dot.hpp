// idist_dot.hpp — the passes behind IDIST_METRIC_DOT (include/idist.h): a DOT index over rows of `dim` coordinates IS the squared-L2
// index over rows of kdim = dim + 1 coordinates, x~ = (x, sqrtf(S - s(x))), searched with q~ = (q, 0); S bounds every finite s(x), so
// |q~ - x~|^2 = |q|^2 + S - 2 q.x orders the rows by descending inner product.  The search, build, brute-force and filter kernels never
// learn about it: they see metric 0 and a kdim-wide index.
//
//   dot_norms_kernel       s(x) of natural [n][dim] rows — row_norm2_group (idist_normalize.hpp), the fold of every distance of this
//                          engine, taken over the dim coordinates — and, for queries, the copy [n][dim + 1] with a trailing 0.
//   dot_max_bits_kernel    the largest bit pattern among the finite entries of s (they are >= +0, so that IS the maximum and no
//                          order of evaluation changes it): every wave reduces its grid-stride share with shuffles and stores ONE
//                          partial; a second launch of the same kernel with one wave reduces the partials.  No atomics.
//   dot_augment_rows_kernel permute_rows_kernel's job for the kdim layout: reads the caller's natural [n][dim] rows, writes [n][stride]
//                          rows in the layout (nb blocks of kdim, natural remainder) with element `dim` = e(x) and zero padding.
//                          stride = kdim, nb = 0 gives natural x~ rows (idist_dot_augment_batch).
//   dot_report_kernel      d -> 0.5f * (d - (s_q[row] + S)) over [nq][width] distances; +inf (padding) and NaN stay as they are.
#pragma once
#include "idist_normalize.hpp"

namespace idist {

__device__ __forceinline__ bool dot_finite(float s) { return (__float_as_uint(s) & 0x7FFFFFFFu) < 0x7F800000u; }
// e(x): one f32 subtraction (>= 0 exactly, S >= s) and a correctly rounded square root; rows that are not finite get 0
__device__ __forceinline__ float dot_extra(float s, float S) { return dot_finite(s) ? __builtin_sqrtf(S - s) : 0.0f; }

// in: natural [n][dim]; out_norm2 (may be nullptr): [n]; out_aug (may be nullptr): [n][dim + 1] = (row, 0).  Eight rows per wave, as in
// normalize_rows_kernel; the copy re-reads the row just read (L2), 32 contiguous bytes per row and step.
__global__ __launch_bounds__(64) void dot_norms_kernel(const float* __restrict__ in, uint32_t n, uint32_t dim,
                                                      float* __restrict__ out_norm2, float* __restrict__ out_aug) {
    const int lane = lane_id(), g = lane >> 3, j = lane & 7;
    const uint32_t groups = (n + 7u) / 8u, kdim = dim + 1u;
    for (uint32_t b = blockIdx.x; b < groups; b += gridDim.x) {
        const uint32_t row = 8u * b + (uint32_t)g;
        const bool on = row < n;
        const float* src = in + (size_t)(on ? row : 0u) * dim;
        const float s0 = row_norm2_group(src, on, dim, 0u, lane);
        if (!on) continue;
        if (out_norm2 && j == 0) out_norm2[row] = s0;
        if (out_aug) {
            float* dst = out_aug + (size_t)row * kdim;
            for (uint32_t e = (uint32_t)j; e < dim; e += 8u) dst[e] = src[e];
            if (j == 0) dst[dim] = 0.0f;
        }
    }
}

// out[blockIdx.x] = the largest bit pattern among the finite entries of s[0..n) this wave visits (0 when there is none)
__global__ __launch_bounds__(64) void dot_max_bits_kernel(const float* __restrict__ s, uint32_t n, uint32_t* __restrict__ out) {
    uint32_t m = 0;
    for (uint32_t i = blockIdx.x * 64u + (uint32_t)lane_id(); i < n; i += gridDim.x * 64u) {
        const float v = s[i];
        const uint32_t bits = __float_as_uint(v);
        if (dot_finite(v) && bits > m) m = bits;
    }
    for (int x = 1; x < 64; x <<= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)m, x, 64);
        m = o > m ? o : m;
    }
    if (lane_id() == 0) out[blockIdx.x] = m;
}

// in: natural [n][dim] (only read); norm2: [n]; out: [n][stride] holding kdim = dim + 1 coordinates in the layout (nb, natural
// remainder), stride >= kdim.  One thread per stored float, as permute_rows_kernel.
__global__ void dot_augment_rows_kernel(const float* __restrict__ in, float* __restrict__ out, uint32_t n, uint32_t dim,
                                        uint32_t stride, uint32_t nb, const float* __restrict__ norm2, float S) {
    const size_t total = (size_t)n * stride;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const uint32_t row = (uint32_t)(idx / stride), o = (uint32_t)(idx % stride);
        const uint32_t e = natural_pos(o, nb);
        float v = 0.0f;
        if (e < dim) v = in[(size_t)row * dim + e];
        else if (e == dim) v = dot_extra(norm2[row], S);
        out[idx] = v;
    }
}

// d: [nq][width]; vec != 0: width % 4 == 0 and d 16-byte aligned (four neighbours then share a row)
__global__ void dot_report_kernel(float* d, const float* __restrict__ s_q, float S, size_t total, uint32_t width, uint32_t vec) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
    auto rep = [](float x, float t) { return (x != x || x == __builtin_inff()) ? x : 0.5f * (x - t); };
    if (vec) {
        for (size_t f = tid; f < total / 4u; f += nth) {
            const float t = s_q[(4u * f) / width] + S;
            float4 v = *reinterpret_cast<const float4*>(d + 4u * f);
            v.x = rep(v.x, t); v.y = rep(v.y, t); v.z = rep(v.z, t); v.w = rep(v.w, t);
            *reinterpret_cast<float4*>(d + 4u * f) = v;
        }
    } else {
        for (size_t i = tid; i < total; i += nth) d[i] = rep(d[i], s_q[i / width] + S);
    }
}

}  // namespace idist
