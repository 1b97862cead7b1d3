// idist_range_allowed.hpp — the kernels where the range search and the restricted search meet
// (idist_search_batch_range_allowed_sets, include/idist.h): every point of a query's own allowed set within its radius.
//
// The answer is DEFINED through what is already bit-exact: the rungs of the range search (idist_range.hpp), each answer filtered by
// the query's bitmap, and an exact scan of the set's rows where the ladder ends — which it does, per query, as soon as a rung's list
// would be longer than the two passes over the set (the end rule).  The walk kernels are not touched; everything here runs between
// their launches, on the launch's stream, wave64, WITHOUT atomics: every buffer holds the same bytes whatever the schedule.  The
// limits, the prefix sums, the close, the sort and the gather are the range search's own kernels, the pending lists
// allowed_pending_kernel with a last rung per query.
//
//   range_allowed_count_kernel   one wave per set: |A_s| (allowed_set_size) and the end rule E[r] < 2 |A_s| in 64-bit integers ->
//                                n_perm[s], the number of rungs the set's queries may run (a prefix of the permitted rungs: E grows).
//   range_allowed_init_kernel    after range_init_kernel: last[q] = n_perm[set of q]; a query whose set is empty is closed as
//                                range_init_kernel left it (rung NONE, count 0).
//   range_allowed_select_kernel  range_select_kernel plus the bitmap: the within-prefix by ballot, then the allowed entries inside it
//                                counted by ballot and popcount.  Saturation is judged on the unrestricted list.
//   range_allowed_copy_kernel    range_copy_kernel plus the bitmap: the first step_cnt[p] allowed entries of the row — they are
//                                the allowed entries of the within-prefix — compacted by prefix popcount into keys.
//   range_allowed_scan_kernel    the exact step: allowed_scan_bits_kernel's window walk (64 windows per load, all-zero ones skipped by
//                                a ballot, set bits compacted into ascending ids in batches of 64, an id that does not fit carried
//                                in its lane's register) around range_scan_kernel's body (dist_rounds, range_within, run twice:
//                                counts per (query, segment), then keys at the offsets of the prefix sum).  Only allowed rows are
//                                fetched; no top-k state.
#pragma once
#include "idist_range.hpp"

namespace idist {

// bits [n_sets][words] -> size [n_sets] = |A_s|, n_perm [n_sets] = the rungs r < lad.n_rungs with E[r] < 2 |A_s|: E is increasing, so
// they are the first n_perm[s] of the ladder.  0 for the empty set and for every set of at most E[0] / 2 points.
__global__ __launch_bounds__(64) void range_allowed_count_kernel(const uint32_t* __restrict__ bits, uint32_t n, uint32_t words,
                                                                 uint32_t n_sets, AllowedLadder lad, uint32_t* __restrict__ size,
                                                                 uint32_t* __restrict__ n_perm) {
    const int lane = lane_id();
    for (uint32_t s = blockIdx.x; s < n_sets; s += gridDim.x) {
        const uint32_t c = allowed_set_size(bits + (size_t)s * words, n, words);
        uint32_t R = 0;
        while (R < lad.n_rungs && (uint64_t)lad.E[R] < 2ull * c) R++;
        if (lane == 0) {
            size[s] = c;
            n_perm[s] = R;
        }
    }
}

// range_init_kernel has run: every query is pending with count 0 and rung NONE.  last [nq]: query q runs the rungs r < last[q].
__global__ void range_allowed_init_kernel(RangeState st, const uint32_t* __restrict__ size, const uint32_t* __restrict__ n_perm,
                                          const uint32_t* __restrict__ set_of, uint32_t* __restrict__ last) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
    for (size_t q = tid; q < st.nq; q += nth) {
        const uint32_t s = set_of[q];
        last[q] = n_perm[s];
        if (size[s] == 0u) st.pending[q] = 0u;
    }
}

// range_select_kernel's arguments and r_pid [np][width]; bits [n_sets][words], set_of [nq]: query q reads the bitmap of its own set.
// step_cnt [np]: the ALLOWED entries of the within-prefix of a query closed here (0 for a saturated one, which stays pending).
__global__ __launch_bounds__(64) void range_allowed_select_kernel(RangeState st, const uint32_t* __restrict__ bits, uint32_t n, uint32_t words,
                                                                  const uint32_t* __restrict__ set_of, const uint32_t* __restrict__ r_pid,
                                                                  const uint32_t* __restrict__ r_dist, const uint32_t* __restrict__ r_count,
                                                                  const uint32_t* __restrict__ r_counters, uint32_t width,
                                                                  const uint32_t* __restrict__ list, uint32_t np, uint32_t rung,
                                                                  uint32_t* __restrict__ step_cnt) {
    const int lane = lane_id();
    for (uint32_t p = blockIdx.x; p < np; p += gridDim.x) {
        const uint32_t q = list ? list[p] : p;
        const uint32_t* b = bits + (size_t)set_of[q] * words;
        uint32_t cnt = r_count[p];
        cnt = cnt < width ? cnt : width;
        const uint32_t* row = r_dist + (size_t)p * width;
        const uint32_t* row_pid = r_pid + (size_t)p * width;
        uint32_t pre = cnt;
        for (uint32_t i0 = 0; i0 < cnt; i0 += 64u) {
            const uint32_t i = i0 + (uint32_t)lane;
            const bool out = i < cnt && !range_within(st.lim, q, row[i]);
            const uint64_t m = __ballot(out);
            if (m) {
                pre = i0 + (uint32_t)__builtin_ctzll(m);
                break;
            }
        }
        uint32_t mine = 0;
        for (uint32_t i0 = 0; i0 < pre; i0 += 64u) {
            const uint32_t i = i0 + (uint32_t)lane;
            const bool ok = i < pre && allowed_bit(b, n, row_pid[i]);
            mine += (uint32_t)__popcll(__ballot(ok));
        }
        if (st.counters && r_counters && lane < 3) st.counters[(size_t)q * 3u + lane] += r_counters[(size_t)p * 3u + lane];
        const bool saturated = cnt == width && pre == cnt;
        if (lane == 0) {
            step_cnt[p] = saturated ? 0u : mine;
            if (!saturated) {
                st.count[q] = mine;
                st.rung[q] = rung;
                st.pending[q] = 0u;
            }
        }
    }
}

// The rows of range_allowed_select_kernel again: a query closed in this step gets its offset and the first step_cnt[p] allowed
// entries of its row as keys from keys + step_off[p] on, in the row's order.  (The within-prefix holds exactly step_cnt[p] allowed
// entries, so they are the first of the row: an allowed entry behind the prefix finds its position taken.)
__global__ __launch_bounds__(64) void range_allowed_copy_kernel(RangeState st, const uint32_t* __restrict__ bits, uint32_t n, uint32_t words,
                                                                const uint32_t* __restrict__ set_of, const uint32_t* __restrict__ r_pid,
                                                                const uint32_t* __restrict__ r_dist, uint32_t width,
                                                                const uint32_t* __restrict__ list, uint32_t np,
                                                                const uint32_t* __restrict__ step_cnt, const uint64_t* __restrict__ step_off,
                                                                uint64_t* __restrict__ keys) {
    const int lane = lane_id();
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint32_t p = blockIdx.x; p < np; p += gridDim.x) {
        const uint32_t q = list ? list[p] : p;
        if (st.pending[q] != 0u) continue;
        const uint32_t* b = bits + (size_t)set_of[q] * words;
        const uint64_t o = step_off[p];
        const uint32_t c = step_cnt[p];
        if (lane == 0) st.off[q] = o;
        uint32_t taken = 0;
        for (uint32_t i0 = 0; i0 < width && taken < c; i0 += 64u) {
            const uint32_t i = i0 + (uint32_t)lane;
            uint32_t id = kInvalid;
            if (i < width) id = r_pid[(size_t)p * width + i];
            const bool ok = i < width && allowed_bit(b, n, id);
            const uint64_t m = __ballot(ok);
            const uint32_t pos = taken + (uint32_t)__popcll(m & below);
            if (ok && pos < c) keys[o + pos] = ((uint64_t)r_dist[(size_t)p * width + i] << 32) | id;
            taken += (uint32_t)__popcll(m);
        }
    }
}

// One batch of the exact step: the na ids in act_pid (ascending) measured, those within the radius of query q counted (the return
// value) and — keys != nullptr — written in act_pid's order from keys + dst on.  Ends with a wave_sync: act_pid is free for the next batch.
template <int NB, int RS, int TAIL>
__device__ __forceinline__ uint32_t range_emit_batch(const IndexView& ix, const Smem& sm, int na, const uint32_t* __restrict__ lim,
                                                     uint32_t q, uint64_t* __restrict__ keys, uint64_t dst) {
    const int lane = lane_id();
    wave_sync();
    dist_rounds<NB, RS, TAIL>(ix, sm.q, sm.act_pid, sm.act_dist, na);
    wave_sync();
    const uint32_t id = lane < na ? sm.act_pid[lane] : kInvalid;
    const uint32_t bits = lane < na ? sm.act_dist[lane] : kNanBits;
    const bool ok = lane < na && range_within(lim, q, bits);
    const uint64_t m = __ballot(ok);
    if (keys && ok) keys[dst + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = ((uint64_t)bits << 32) | id;
    wave_sync();
    return (uint32_t)__popcll(m);
}

// The exact step, straight from the bitmaps.  bits [n_sets][words]; queries [np][dim]: the pending queries' rows; list [np] (nullptr:
// the identity): their original indices, set_of [nq]: their sets.  The n_win = ceil(n / 64) windows of [0, n) are cut into S contiguous
// segments [n_win s / S, n_win (s + 1) / S) (an empty one yields no hit); work item w = p * S + s.  keys == nullptr: seg_cnt[w] = the
// hits of the item.  Otherwise the hits are written, ascending id, from keys + seg_off[w] on (seg_off: the prefix sum of the first
// run).  Ids are < n (allowed_window clears the bits beyond) and reach act_pid ascending, so neither S nor the batches show.
template <int NB, int RS, int TAIL>
__global__ __launch_bounds__(64) void range_allowed_scan_kernel(IndexView ix, const float* __restrict__ queries, uint32_t np,
                                                                const uint32_t* __restrict__ bits, uint32_t n, uint32_t words,
                                                                const uint32_t* __restrict__ list, const uint32_t* __restrict__ set_of,
                                                                const uint32_t* __restrict__ lim, uint32_t S,
                                                                uint32_t* __restrict__ seg_cnt, const uint64_t* __restrict__ seg_off,
                                                                uint64_t* __restrict__ keys) {
    IDIST_DYN_SMEM(smem_raw);
    const Smem sm = carve(smem_raw, ix.stride, 0, false);
    const int lane = lane_id();
    const uint64_t below = (1ull << lane) - 1ull;
    const uint32_t n_win = (uint32_t)(((uint64_t)n + 63u) / 64u);
    const uint64_t items = (uint64_t)np * S;
    for (uint64_t w = blockIdx.x; w < items; w += gridDim.x) {
        uint32_t p, lo, hi;
        scan_segment(n_win, S, w, &p, &lo, &hi);
        const uint32_t q = list ? list[p] : p;
        const uint32_t* b = bits + (size_t)set_of[q] * words;
        stage_query<NB>(ix, sm.q, queries + (size_t)p * ix.dim);
        const uint64_t dst = keys ? seg_off[w] : 0ull;
        uint32_t taken = 0;
        uint32_t fill = 0;                                    // ids waiting in act_pid, < 64 between windows
        for (uint32_t g = lo; g < hi; g += 64u) {
            const uint32_t mine = g + (uint32_t)lane;         // lane j holds window g + j
            const uint64_t win = mine < hi ? allowed_window(b, n, words, mine) : 0ull;
            uint64_t nz = __ballot(win != 0ull);
            while (nz) {
                const int j = __builtin_ctzll(nz);
                nz &= nz - 1ull;
                // (j comes from a ballot: wave-uniform, so the window travels through scalar registers and `fill` stays uniform)
                const uint64_t m = ((uint64_t)readlane_u32((uint32_t)(win >> 32), j) << 32) | readlane_u32((uint32_t)win, j);
                const bool on = ((m >> lane) & 1ull) != 0ull;
                const uint32_t id = (g + (uint32_t)j) * 64u + (uint32_t)lane;
                const uint32_t pos = fill + (uint32_t)__popcll(m & below);
                if (on && pos < 64u) sm.act_pid[pos] = id;
                fill += (uint32_t)__popcll(m);
                if (fill >= 64u) {
                    taken += range_emit_batch<NB, RS, TAIL>(ix, sm, 64, lim, q, keys, dst + taken);
                    if (on && pos >= 64u) sm.act_pid[pos - 64u] = id;     // carried over in the lane's register
                    fill -= 64u;
                }
            }
        }
        if (fill) taken += range_emit_batch<NB, RS, TAIL>(ix, sm, (int)fill, lim, q, keys, dst + taken);
        if (!keys && lane == 0) seg_cnt[w] = taken;
    }
}

}  // namespace idist
