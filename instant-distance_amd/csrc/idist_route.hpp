// idist_route.hpp — routed search over a partitioned index: every query goes to the `nprobe` non-empty parts whose centroids are
// nearest, instead of to all of them (idist_partitioned_search_batch_routed).
//
//   route_kernel          one wave per query: the canonical squared-L2 distance (the eight FMA chains of idist_device.hpp and their
//                         fold, over natural rows) of the prepared query to the <= 64 centroids, eight centroids per pass; lane p then
//                         holds the key  distance bits << 32 | p  of part p and its rank is the number of smaller keys (the
//                         reference's `Candidate` order: distance, NaN greatest, then the part).  Ranks below nprobe are the route.
//                         It also clears the staging counts of EVERY (part, query) pair: the scatter below fills in the routed ones,
//                         and the merge ignores a list whose count is 0.
//   route_lists_kernel    one wave per part: the queries routed to it, in query order — a ballot and a running offset, no atomics.
//   route_gather_kernel   on the part's device: its queries packed densely, [m][kdim].
//   route_scatter_kernel  on the merge device: the parts' dense result rows back to the rows of their queries in the [P][nq][ef]
//                         staging memory the merge reads.
// Every word is written by exactly one lane, whatever the grid.
#pragma once
#include "idist_device.hpp"

namespace idist {

constexpr uint32_t kRouteMaxParts = 64;

struct RouteArgs {
    const float* Q;            // [nq][kdim] prepared queries
    const float* cent;         // [P][kdim]
    uint32_t nq, kdim, P, nprobe;
    uint64_t nonempty;         // bit p: part p holds points
    uint32_t* route;           // [nq][nprobe], padded with kInvalid
    uint32_t* sel;             // [P][nq] 1: the query goes to the part
    uint32_t* s_cnt;           // [P][nq] staging counts, cleared
    uint32_t* s_ctr;           // [P][nq][3] staging counters, cleared; or nullptr
};

__global__ __launch_bounds__(64) void route_kernel(RouteArgs a) {
    IDIST_DYN_SMEM(smem_raw);
    float* q_s = reinterpret_cast<float*>(smem_raw);                      // [kdim]
    uint32_t* dist_s = reinterpret_cast<uint32_t*>(q_s + ((a.kdim + 3u) & ~3u));   // [64]
    const int lane = lane_id();
    const uint32_t g = (uint32_t)lane >> 3, j = (uint32_t)lane & 7u;
    const uint32_t dp = (a.kdim + 3u) & ~3u, steps = dp / 8u;             // the row padded with zeros to a multiple of four
    const bool tail = (dp & 7u) == 4u;
    const uint32_t ne = (uint32_t)__popcll(a.nonempty), nr = ne < a.nprobe ? ne : a.nprobe;
    for (uint32_t q = blockIdx.x; q < a.nq; q += gridDim.x) {
        wave_sync();                                                      // the previous query is done with q_s / dist_s
        for (uint32_t e = (uint32_t)lane; e < a.kdim; e += 64u) q_s[e] = a.Q[(size_t)q * a.kdim + e];
        wave_sync();
        for (uint32_t c0 = 0; c0 < a.P; c0 += 8u) {                       // group g: centroid c0 + g, lane j of it: chain j
            const uint32_t c = c0 + g;
            const float* row = a.cent + (size_t)(c < a.P ? c : 0u) * a.kdim;
            float acc = 0.0f;
            for (uint32_t s = 0; s < steps; s++) {
                const uint32_t i = 8u * s + j;
                const float d = i < a.kdim ? q_s[i] - row[i] : 0.0f;
                acc = __builtin_fmaf(d, d, acc);
            }
            const uint32_t it = 8u * steps + (j & 3u);
            const bool ht = tail && it < a.kdim;
            const float res = fold_chains(acc, tail, ht ? q_s[it] : 0.0f, ht ? row[it] : 0.0f);
            if (j == 0u && c < a.P) dist_s[c] = canon_bits(res, 0u);
        }
        wave_sync();
        const bool valid = (uint32_t)lane < a.P && ((a.nonempty >> lane) & 1ull);
        const uint64_t key = valid ? ((uint64_t)dist_s[lane] << 32) | (uint64_t)lane : ~0ull;
        uint32_t rank = 0;
        for (uint32_t s = 0; s < a.P; s++) rank += bcast_u64(key, (int)s) < key ? 1u : 0u;
        const bool take = valid && rank < a.nprobe;
        if (take) a.route[(size_t)q * a.nprobe + rank] = (uint32_t)lane;
        if ((uint32_t)lane >= nr && (uint32_t)lane < a.nprobe) a.route[(size_t)q * a.nprobe + lane] = kInvalid;
        if ((uint32_t)lane < a.P) {
            const size_t o = (size_t)lane * a.nq + q;
            a.sel[o] = take ? 1u : 0u;
            a.s_cnt[o] = 0u;
            if (a.s_ctr) { a.s_ctr[o * 3u] = 0u; a.s_ctr[o * 3u + 1u] = 0u; a.s_ctr[o * 3u + 2u] = 0u; }
        }
    }
}

// list[p][0 .. lens[p]) = the queries with sel[p][q], ascending
__global__ __launch_bounds__(64) void route_lists_kernel(const uint32_t* __restrict__ sel, uint32_t P, uint32_t nq, uint32_t* __restrict__ list,
                                                        uint32_t* __restrict__ lens) {
    const int lane = lane_id();
    for (uint32_t p = blockIdx.x; p < P; p += gridDim.x) {
        uint32_t off = 0;
        for (uint32_t base = 0; base < nq; base += 64u) {
            const uint32_t q = base + (uint32_t)lane;
            const bool f = q < nq && sel[(size_t)p * nq + q] != 0u;
            const uint64_t m = __ballot(f);
            if (f) list[(size_t)p * nq + off + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = q;
            off += (uint32_t)__popcll(m);
        }
        if (lane == 0) lens[p] = off;
    }
}

// out[i] = Q[list[i]] for i < m, rows of kdim floats (one wave per row)
__global__ __launch_bounds__(64) void route_gather_kernel(const float* __restrict__ Q, const uint32_t* __restrict__ list, uint32_t m,
                                                         uint32_t kdim, float* __restrict__ out) {
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = blockIdx.x; i < m; i += gridDim.x) {
        const float* src = Q + (size_t)list[i] * kdim;
        for (uint32_t e = lane; e < kdim; e += 64u) out[(size_t)i * kdim + e] = src[e];
    }
}

struct ScatterArgs {
    const uint32_t* g_pid;     // [total][ef] the parts' dense rows, part p's from row off[p]
    const uint32_t* g_dist;
    const uint32_t* g_cnt;     // [total]
    const uint32_t* g_ctr;     // [total][3] or nullptr
    const uint32_t* list;      // [P][nq]
    uint32_t P, nq, ef;
    uint32_t* s_pid;           // [P][nq][ef]
    uint32_t* s_dist;
    uint32_t* s_cnt;           // [P][nq]
    uint32_t* s_ctr;           // [P][nq][3]
    uint32_t off[kRouteMaxParts + 1];
};

__global__ __launch_bounds__(64) void route_scatter_kernel(ScatterArgs a) {
    const int lane = lane_id();
    const uint32_t lo = (uint32_t)lane < a.P ? a.off[lane] : 0u, hi = (uint32_t)lane < a.P ? a.off[lane + 1] : 0u;
    for (uint32_t d = blockIdx.x; d < a.off[a.P]; d += gridDim.x) {
        const uint32_t p = (uint32_t)__builtin_ctzll(__ballot(lo <= d && d < hi));      // exactly one part holds dense row d
        const uint32_t q = a.list[(size_t)p * a.nq + (d - a.off[p])];
        const size_t dst = (size_t)p * a.nq + q;
        for (uint32_t i = (uint32_t)lane; i < a.ef; i += 64u) {
            a.s_pid[dst * a.ef + i] = a.g_pid[(size_t)d * a.ef + i];
            a.s_dist[dst * a.ef + i] = a.g_dist[(size_t)d * a.ef + i];
        }
        if (lane == 0) a.s_cnt[dst] = a.g_cnt[d];
        if (a.g_ctr && lane < 3) a.s_ctr[dst * 3u + lane] = a.g_ctr[(size_t)d * 3u + lane];
    }
}

}  // namespace idist
