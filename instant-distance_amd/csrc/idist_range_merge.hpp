// idist_range_merge.hpp — the union step of a range search over a partitioned index (idist_partitioned_search_batch_range,
// include/idist.h): per query P ascending key lists of ANY length -> one ascending list, global ids, reported
// distances.
//
// merge_topk_kernel (idist_merge.hpp) merges P lists of one fixed width into a fixed width, one wave per query, staged in LDS.  A
// range result is P lists of 0 ... n_p keys per query, their total known only when the parts have answered, and one query's lists
// can be ten thousand times longer than its neighbour's.  The idea is that kernel's, with no cut and no width: every list is
// ascending in the key  raw distance bits << 32 | global id  and keys of different lists are distinct, so
//     rank = (the key's index in its own list) + sum over the other lists of the query of (number of keys below it),
// each term one binary search, and the element stores itself at lims[q] + rank as a global id and a reported distance (the report
// of range_gather_kernel, with the query's own term): no gather pass behind it.  Rules of idist_range.hpp: wave64, NO atomics, every
// buffer holds the same bytes whatever the schedule, the lists' COUNTS rule, never padding.  Nothing is staged: the lists are read
// where the parts' searches left them (completion order, a per-query offset and count), there is no size cap and no LDS.
//
//   range_merge_counts_kernel   c[q] = the sum over the lists of their counts for q, the counters summed with them; lims is the
//                               exclusive prefix sum of c (range_chunk_sums_kernel / range_offsets_kernel of idist_range.hpp).
//   range_merge_kernel          work is divided by RESULTS, not by queries: wave w owns the elements [w * tile, (w + 1) * tile) of
//                               the batch in the order (query, list, index in the list) — a pass that gives each query to one wave
//                               runs as long as its most loaded wave, and here a query that ended in an exact scan with 50,000
//                               hits sits beside hundreds with 3.  An element finds its query by bisection over lims (the lists of
//                               a query hold lims[q + 1] - lims[q] keys together, so lims numbers the inputs as well as the
//                               outputs), between the tile's first and last query; its list by walking the query's counts.
#pragma once
#include "idist_merge.hpp"
#include "idist_range.hpp"

namespace idist {

constexpr uint32_t kRangeMergeTile = 256;          // elements a wave owns at a time: four rounds of 64

// The lists of one call, by value in the kernel arguments (2.3 KB): list l holds, for query q, cnt[l][q] keys
// dist_bits << 32 | local id  at keys[l] + off[l][q], ascending; its global ids are base[l] + local id.
struct RangeLists {
    const uint64_t* keys[kMergeMaxLists];
    const uint64_t* off[kMergeMaxLists];           // [nq]
    const uint32_t* cnt[kMergeMaxLists];           // [nq]
    const uint32_t* ctr[kMergeMaxLists];           // [nq][3] or nullptr (range_merge_counts_kernel alone reads it)
    uint32_t base[kMergeMaxLists];
    uint32_t n_lists, nq;
};

// One lane per query.  out_ctr [nq][3] or nullptr.
__global__ void range_merge_counts_kernel(RangeLists L, uint32_t* __restrict__ c, uint32_t* __restrict__ out_ctr) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
    for (size_t q = tid; q < L.nq; q += nth) {
        uint32_t s = 0, c0 = 0, c1 = 0, c2 = 0;
        for (uint32_t l = 0; l < L.n_lists; l++) {
            s += L.cnt[l][q];
            if (out_ctr && L.ctr[l]) {
                const uint32_t* t = L.ctr[l] + q * 3u;
                c0 += t[0]; c1 += t[1]; c2 += t[2];
            }
        }
        c[q] = s;
        if (out_ctr) { out_ctr[q * 3u] = c0; out_ctr[q * 3u + 1u] = c1; out_ctr[q * 3u + 2u] = c2; }
    }
}

// the query that owns element e: the largest q of [lo, hi] with lims[q] <= e (lims[lo] <= e holds; a query without results owns nothing)
__device__ __forceinline__ uint32_t range_merge_owner(const uint64_t* __restrict__ lims, uint32_t lo, uint32_t hi, uint64_t e) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1u) / 2u;
        if (lims[mid] <= e) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

// lims [nq + 1]: the prefix sum of the counts pass, total = lims[nq] > 0; tile: a multiple of 64.  s_q [nq]: s(q) (DOT only), S: the
// bound the parts share — the term of the report is s_q[q] + S, range_init_kernel's.  out_pid / out_dist [total].
__global__ __launch_bounds__(64) void range_merge_kernel(RangeLists L, const uint64_t* __restrict__ lims, uint64_t total, uint32_t tile,
                                                         uint32_t metric, const float* __restrict__ s_q, float S,
                                                         uint32_t* __restrict__ out_pid, float* __restrict__ out_dist) {
    const int lane = lane_id();
    const uint32_t P = L.n_lists, last = L.nq - 1u;
    const uint64_t tiles = (total + tile - 1u) / tile;
    for (uint64_t w = blockIdx.x; w < tiles; w += gridDim.x) {
        const uint64_t e0 = w * tile, e1 = e0 + tile < total ? e0 + tile : total;
        const uint32_t qa = range_merge_owner(lims, 0u, last, e0), qb = range_merge_owner(lims, qa, last, e1 - 1u);   // wave-uniform
        for (uint64_t e = e0 + (uint64_t)lane; e < e1; e += 64u) {
            const uint32_t q = range_merge_owner(lims, qa, qb, e);
            const uint64_t first = lims[q];
            uint32_t i = (uint32_t)(e - first), mine = P;            // index among the query's keys, then in its own list
            uint64_t key = 0;
            for (uint32_t l = 0; l < P; l++) {
                const uint32_t c = L.cnt[l][q];
                if (i < c) {
                    key = L.keys[l][L.off[l][q] + i] + (uint64_t)L.base[l];      // (base + id fits 32 bits: no carry into the distance)
                    mine = l;
                    break;
                }
                i -= c;
            }
            if (mine == P) continue;                                 // (counts that changed behind lims: nothing is stored)
            uint64_t rank = i;
            for (uint32_t l = 0; l < P; l++) {
                if (l == mine) continue;
                uint32_t lo = 0, hi = L.cnt[l][q];                   // number of keys of list l below mine (keys are distinct)
                if (hi == 0u) continue;
                const uint64_t* a = L.keys[l] + L.off[l][q];
                const uint64_t b = (uint64_t)L.base[l];
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (a[mid] + b < key) lo = mid + 1u;
                    else hi = mid;
                }
                rank += lo;
            }
            const float t = metric == kRangeDot ? s_q[q] + S : 0.0f;
            out_pid[first + rank] = (uint32_t)key;
            out_dist[first + rank] = range_report(metric, __uint_as_float((uint32_t)(key >> 32)), t);
        }
    }
}

}  // namespace idist
