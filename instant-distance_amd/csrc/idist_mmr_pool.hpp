// idist_mmr_pool.hpp — the row pool of the diverse search over a partitioned index (idist_partitioned_search_batch_mmr, include/idist.h;
// DESIGN.md §8.1).  The selection needs pair distances between stored rows that live in different parts, possibly on different GPUs;
// mmr_tile_kernel and mmr_global_kernel address rows of ONE array.  So, after the merge, the rows behind the first
// m = min(count, fetch) entries of every query's merged list are copied, still in stored blocked order (`stride` floats), into one
// dense buffer on the merge device,
//
//     pool[slot][stride],        row_of[q * fetch + pos] = slot        (kInvalid: position pos is beyond m, or its id beyond N)
//
// and the selection kernels (POOL = true, idist_mmr.hpp) read rows by slot.  Slots are PART-MAJOR — all of part 0's rows, query by
// query and in list order inside a query, then part 1's — so that a part's rows form one contiguous range and travel in one copy.
//
//   mmr_pool_lists_kernel<false>  the count pass, on the merge device, one wave per query: cnt[p][q] = the pool positions of q whose
//                                 global id falls into part p (base[0..P] in LDS, a binary search per position).
//   (range_chunk_sums_kernel / range_offsets_kernel of idist_range.hpp: off = the exclusive prefix sum over the P * nq counts)
//   mmr_pool_lists_kernel<true>   the fill pass, the same walk: lid[off[p][q] + j] = the LOCAL id of the j-th position of q in part p,
//                                 row_of[q][pos] = that slot.  Lane p of the wave carries part p's next free slot (P <= 64 = the wave);
//                                 the order inside a batch of 64 positions comes from a ballot per distinct part and a popcount.
//                                 No atomics: every word is written by exactly one lane, the same bytes on every grid.
//   mmr_pool_gather_kernel        on each part's device and stream: dst[i] = the part's stored row list[i].  Eight lanes per row, 16-byte
//                                 loads and stores over the whole stride, four of them requested per lane before the first is stored
//                                 (32 rows per workgroup, 8 per wave, in flight), grid-stride over the rows.
#pragma once
#include "idist_merge.hpp"   // kMergeMaxLists

namespace idist {

struct PoolArgs {
    const uint32_t* r_pid;    // [nq][width] the merged lists: global ids
    const uint32_t* r_count;  // [nq]
    uint32_t nq, width, fetch, P;
    uint32_t* cnt;            // [P][nq]      count pass: the pool positions of query q in part p
    const uint64_t* off;      // [P * nq + 1] fill pass: the exclusive prefix sum of cnt (part-major)
    uint32_t* lid;            // [slots]      fill pass: the local id behind every slot
    uint32_t* row_of;         // [nq][fetch]  fill pass: the slot of every pool position
    uint64_t* bounds;         // [P + 1]      fill pass: off[p * nq], the first slot of every part; bounds[P] = slots
    uint32_t base[kMergeMaxLists + 1];   // part p holds the global ids base[p] .. base[p + 1] - 1
};

constexpr size_t kPoolListsSmem = (kMergeMaxLists + 4) * 4;   // base[0..P], P <= 64

template <bool FILL>
__global__ __launch_bounds__(64) void mmr_pool_lists_kernel(PoolArgs a) {
    IDIST_DYN_SMEM(smem_raw);
    uint32_t* base_s = reinterpret_cast<uint32_t*>(smem_raw);
    const int lane = lane_id();
    const uint64_t below = (1ull << lane) - 1ull;
    const uint32_t P = a.P, nq = a.nq;
    for (uint32_t i = (uint32_t)lane; i <= P; i += 64u) base_s[i] = a.base[i];
    wave_sync();
    if (FILL && blockIdx.x == 0)
        for (uint32_t i = (uint32_t)lane; i <= P; i += 64u) a.bounds[i] = a.off[(size_t)i * nq];
    for (uint32_t q = blockIdx.x; q < nq; q += gridDim.x) {
        uint32_t c = a.r_count[q];
        c = c < a.width ? c : a.width;
        const uint32_t m = c < a.fetch ? c : a.fetch;
        // lane p: the next free slot of part p (FILL), the positions counted for it so far (count pass)
        uint32_t run = FILL && (uint32_t)lane < P ? (uint32_t)a.off[(size_t)lane * nq + q] : 0u;
        for (uint32_t b = 0; b < (FILL ? a.fetch : m); b += 64u) {
            const uint32_t pos = b + (uint32_t)lane;
            uint32_t part = P, gid = 0u;
            if (pos < m) {
                gid = a.r_pid[(size_t)q * a.width + pos];
                // part = the number of i in 1..P with base[i] <= gid (empty parts fall out by themselves); P: an id >= N, no part
                uint32_t lo = 0u, hi = P;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (base_s[mid + 1u] <= gid) lo = mid + 1u;
                    else hi = mid;
                }
                part = lo;
            }
            const bool in = part < P;
            if (FILL && pos < a.fetch && !in) a.row_of[(size_t)q * a.fetch + pos] = kInvalid;
            uint64_t todo = __ballot(in);
            while (todo) {                                         // once per distinct part of the batch; everything here is wave-uniform
                const uint32_t p = bcast_u32(part, __builtin_ctzll(todo));
                const bool mine = in && part == p;
                const uint64_t same = __ballot(mine);
                const uint32_t first = bcast_u32(run, (int)p);
                if (FILL && mine) {
                    const uint32_t slot = first + (uint32_t)__popcll(same & below);
                    a.lid[slot] = gid - base_s[p];
                    a.row_of[(size_t)q * a.fetch + pos] = slot;
                }
                if ((uint32_t)lane == p) run += (uint32_t)__popcll(same);
                todo &= ~same;
            }
        }
        if (!FILL && (uint32_t)lane < P) a.cnt[(size_t)lane * nq + q] = run;
    }
}

// dst[i][0 .. stride) = part.points[list[i]][0 .. stride) for i < m.  stride is a multiple of 16 floats and both arrays start on a
// 16-byte boundary, so a row is stride / 4 float4 pieces; lane j of an eight-lane group moves the pieces j, j + 8, ...
__global__ __launch_bounds__(256) void mmr_pool_gather_kernel(IndexView part, const uint32_t* __restrict__ list, uint32_t m, float* __restrict__ dst) {
    const uint32_t g = threadIdx.x >> 3, j = threadIdx.x & 7u;
    const uint32_t pieces = part.stride >> 2;
    for (uint64_t i = (uint64_t)blockIdx.x * 32u + g; i < m; i += (uint64_t)gridDim.x * 32u) {
        const uint32_t id = list[i];
        if (id >= part.n) continue;                                // (never: the lists hold ids of this part)
        const float* src = part.points + (size_t)id * part.stride;
        float* out = dst + (size_t)i * part.stride;
        for (uint32_t c0 = j; c0 < pieces; c0 += 32u) {
            float4 v[4];
#pragma unroll
            for (uint32_t u = 0; u < 4u; u++)
                if (c0 + 8u * u < pieces) v[u] = ldg_row4(src + (size_t)(c0 + 8u * u) * 4u);
#pragma unroll
            for (uint32_t u = 0; u < 4u; u++)
                if (c0 + 8u * u < pieces) *reinterpret_cast<float4*>(out + (size_t)(c0 + 8u * u) * 4u) = v[u];
        }
    }
}

}  // namespace idist
