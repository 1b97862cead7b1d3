// idist_range.hpp — the kernels around a range search (idist_search_batch_range, include/idist.h).
//
// A range search is DEFINED through what is already bit-exact, as the restricted search is (idist_allowed.hpp): Hnsw::search at
// growing ef_search (the "rungs") while a rung's list is full and wholly within the radius, and an exact scan of every row where
// the ladder ends.  The walk kernels are not touched; everything here runs between their launches, on the launch's stream, wave64,
// WITHOUT atomics: every buffer holds the same bytes whatever the schedule.
//
//   range_init_kernel        per query: "within" as a test on RAW distance bits (range_limit: a bisection over the bit patterns
//                            +0 ... FLT_MAX with the report arithmetic of the report kernels, +inf tested on its own), the term of the
//                            metric's report, count 0, rung NONE, counters 0, pending.
//   range_select_kernel      one wave per pending query: the length of the within-prefix of its rung row by ballot in chunks of 64,
//                            the rung's counters added; a row that is full and wholly within stays pending, any other closes the query.
//   range_chunk_sums_kernel  \ an exclusive u64 prefix sum over u32 counts in two levels: the sum of every chunk of 64 items, then
//   range_offsets_kernel     / per chunk the chunk sums in front of it are counted (allowed_pending_kernel's scheme: no look-back).
//   range_copy_kernel        the prefixes closed in this step as keys dist_bits << 32 | pid at their offsets in the result buffer.
//   range_scan_kernel        the exact step: grid = pending queries x S contiguous segments of [0, n) (scan_segment, stage_query: the
//                            exact scans' shared steps, idist_device.hpp), dist_rounds on 64 consecutive ids at a time.  Run twice:
//                            the first run stores the number of hits per (query, segment), the second writes the keys at the offsets
//                            the prefix sum gave, ascending id within a segment.  No top-k.
//   range_close_kernel       the exact queries closed: count, offset, rung EXACT.
//   range_sort_kernel        every exact query's keys ascending, in place: a bitonic network of ASCENDING comparators only (a merge
//                            level = one "flip" i <-> k - 1 - i, then half-cleaners i <-> i + j), so a comparator whose upper end lies
//                            beyond the list can simply be left out: any length, no padding in memory.  Strides below the chunk
//                            run in LDS (one wave per chunk), the longer ones in global memory, one launch per stride.
//   range_gather_kernel      fetch: per query its keys from where it was closed (completion order) to [lims[q], lims[q + 1]), split
//                            into pid and distance, the metric's report applied with the query's own term.
#pragma once
#include "idist_allowed.hpp"

namespace idist {

constexpr uint32_t kRangeCosine = 2u;    // IDIST_METRIC_COSINE
constexpr uint32_t kRangeDot = 4u;       // IDIST_METRIC_DOT
constexpr uint32_t kInfBits = 0x7f800000u;

// what the metric reports for the raw distance x: scale_half_kernel's and dot_report_kernel's arithmetic, the identity otherwise
__device__ __forceinline__ float range_report(uint32_t metric, float x, float t) {
    if (metric == kRangeCosine) return x != x ? x : 0.5f * x;
    if (metric == kRangeDot) return (x != x || x == __builtin_inff()) ? x : 0.5f * (x - t);
    return x;
}

struct RangeState {
    uint32_t* lim;        // [nq][2]: raw bits b are within iff b < lim[0] || b == lim[1]
    float* term;          // [nq] DOT: s(q) + S, else 0
    uint32_t* count;      // [nq]
    uint64_t* off;        // [nq] where the query's keys start in the result buffer
    uint32_t* rung;       // [nq]
    uint32_t* counters;   // [nq][3] or nullptr
    uint32_t* pending;    // [nq] 1: not answered yet
    uint32_t nq;
};

__device__ __forceinline__ bool range_within(const uint32_t* __restrict__ lim, uint32_t q, uint32_t bits) {
    return bits < lim[2u * q] || bits == lim[2u * q + 1u];
}

// The number of finite patterns +0 ... FLT_MAX whose report is <= r: the report is non-decreasing in the raw distance, so they are
// a prefix and 31 halvings find its length.
__device__ __forceinline__ uint32_t range_limit(uint32_t metric, float t, float r) {
    uint32_t lo = 0u, hi = kInfBits;                          // patterns < lo are within, patterns >= hi are not
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (range_report(metric, __uint_as_float(mid), t) <= r) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// radius [n_radius] (1: shared); s_q [nq] (DOT only).  One lane per query.
__global__ void range_init_kernel(RangeState st, const float* __restrict__ radius, uint32_t n_radius, uint32_t metric,
                                  const float* __restrict__ s_q, float S) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
    for (size_t q = tid; q < st.nq; q += nth) {
        const float r = radius[n_radius == 1u ? 0u : q];
        const float t = metric == kRangeDot ? s_q[q] + S : 0.0f;
        st.term[q] = t;
        st.lim[2u * q] = range_limit(metric, t, r);
        st.lim[2u * q + 1u] = range_report(metric, __uint_as_float(kInfBits), t) <= r ? kInfBits : 0xFFFFFFFFu;
        st.count[q] = 0u;
        st.off[q] = 0ull;
        st.rung[q] = kRungNone;
        st.pending[q] = 1u;
        if (st.counters) { st.counters[3 * q] = 0u; st.counters[3 * q + 1] = 0u; st.counters[3 * q + 2] = 0u; }
    }
}

// r_dist [np][width] / r_count [np] / r_counters [np][3] or nullptr: the rung's rows of the np pending queries; list [np]: their
// original indices (nullptr: the identity).  step_cnt [np]: the entries a query closed here contributes to the result (0 otherwise).
__global__ __launch_bounds__(64) void range_select_kernel(RangeState st, const uint32_t* __restrict__ r_dist,
                                                          const uint32_t* __restrict__ r_count, const uint32_t* __restrict__ r_counters,
                                                          uint32_t width, const uint32_t* __restrict__ list, uint32_t np, uint32_t rung,
                                                          uint32_t* __restrict__ step_cnt) {
    const int lane = lane_id();
    for (uint32_t p = blockIdx.x; p < np; p += gridDim.x) {
        const uint32_t q = list ? list[p] : p;
        uint32_t cnt = r_count[p];
        cnt = cnt < width ? cnt : width;
        const uint32_t* row = r_dist + (size_t)p * width;
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
        if (st.counters && r_counters && lane < 3) st.counters[(size_t)q * 3u + lane] += r_counters[(size_t)p * 3u + lane];
        const bool saturated = cnt == width && pre == cnt;
        if (lane == 0) {
            step_cnt[p] = saturated ? 0u : pre;
            if (!saturated) {
                st.count[q] = pre;
                st.rung[q] = rung;
                st.pending[q] = 0u;
            }
        }
    }
}

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src) { return bcast_u64(v, src); }
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

// cnt [N] -> chunk_sum [ceil(N / 64)]: wave b sums the items [64 b, 64 b + 64).
__global__ __launch_bounds__(64) void range_chunk_sums_kernel(const uint32_t* __restrict__ cnt, uint64_t N, uint64_t* __restrict__ chunk_sum) {
    const int lane = lane_id();
    const uint64_t chunks = (N + 63u) / 64u;
    for (uint64_t b = blockIdx.x; b < chunks; b += gridDim.x) {
        const uint64_t i = 64u * b + (uint64_t)lane;
        const uint64_t s = wave_sum_u64(i < N ? (uint64_t)cnt[i] : 0ull);
        if (lane == 0) chunk_sum[b] = s;
    }
}

// off [N + 1]: off[i] = base + cnt[0] + ... + cnt[i - 1]; off[N] is the new total.
__global__ __launch_bounds__(64) void range_offsets_kernel(const uint32_t* __restrict__ cnt, uint64_t N, const uint64_t* __restrict__ chunk_sum,
                                                           uint64_t base, uint64_t* __restrict__ off) {
    const int lane = lane_id();
    const uint64_t chunks = (N + 63u) / 64u;
    for (uint64_t b = blockIdx.x; b < chunks; b += gridDim.x) {
        uint64_t before = 0;
        for (uint64_t c = (uint64_t)lane; c < b; c += 64u) before += chunk_sum[c];
        before = wave_sum_u64(before) + base;
        const uint64_t i = 64u * b + (uint64_t)lane;
        const uint64_t mine = i < N ? (uint64_t)cnt[i] : 0ull;
        uint64_t incl = mine;                                  // inclusive scan over the wave
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t o = shfl_u64(incl, lane >= d ? lane - d : lane);
            if (lane >= d) incl += o;
        }
        if (i < N) off[i] = before + incl - mine;
        if (b + 1u == chunks && lane == 63) off[N] = before + incl;
    }
}

// The rows of range_select_kernel again: a query closed in this step (it was in `list`, it is no longer pending) gets its offset and
// its step_cnt[p] first entries as keys at keys + step_off[p].
__global__ __launch_bounds__(64) void range_copy_kernel(RangeState st, const uint32_t* __restrict__ r_pid, const uint32_t* __restrict__ r_dist,
                                                        uint32_t width, const uint32_t* __restrict__ list, uint32_t np,
                                                        const uint32_t* __restrict__ step_cnt, const uint64_t* __restrict__ step_off,
                                                        uint64_t* __restrict__ keys) {
    const int lane = lane_id();
    for (uint32_t p = blockIdx.x; p < np; p += gridDim.x) {
        const uint32_t q = list ? list[p] : p;
        if (st.pending[q] != 0u) continue;
        const uint64_t o = step_off[p];
        const uint32_t c = step_cnt[p];
        if (lane == 0) st.off[q] = o;
        for (uint32_t i = (uint32_t)lane; i < c; i += 64u)
            keys[o + i] = ((uint64_t)r_dist[(size_t)p * width + i] << 32) | r_pid[(size_t)p * width + i];
    }
}

// The exact step.  [0, n) cut into S contiguous segments [n s / S, n (s + 1) / S); work item w = p * S + s.  queries [np][dim]: the
// pending queries' rows; list [np]: their original indices (nullptr: the identity).  keys == nullptr: seg_cnt[w] = the hits of the
// item.  Otherwise the hits are written, ascending id, from keys + seg_off[w] on (seg_off: the prefix sum of the first run).
template <int NB, int RS, int TAIL>
__global__ __launch_bounds__(64) void range_scan_kernel(IndexView ix, const float* __restrict__ queries, uint32_t np,
                                                        const uint32_t* __restrict__ list, const uint32_t* __restrict__ lim, uint32_t S,
                                                        uint32_t* __restrict__ seg_cnt, const uint64_t* __restrict__ seg_off,
                                                        uint64_t* __restrict__ keys) {
    IDIST_DYN_SMEM(smem_raw);
    const Smem sm = carve(smem_raw, ix.stride, 0, false);
    const int lane = lane_id();
    const uint64_t below = (1ull << lane) - 1ull;
    const uint64_t items = (uint64_t)np * S;
    for (uint64_t w = blockIdx.x; w < items; w += gridDim.x) {
        uint32_t p, lo, hi;
        scan_segment(ix.n, S, w, &p, &lo, &hi);
        const uint32_t q = list ? list[p] : p;
        stage_query<NB>(ix, sm.q, queries + (size_t)p * ix.dim);
        const uint64_t dst = keys ? seg_off[w] : 0ull;
        uint32_t taken = 0;
        for (uint32_t base = lo; base < hi; base += 64u) {
            const int na = hi - base < 64u ? (int)(hi - base) : 64;
            const uint32_t id = base + (uint32_t)lane;
            if (lane < na) sm.act_pid[lane] = id;
            wave_sync();
            dist_rounds<NB, RS, TAIL>(ix, sm.q, sm.act_pid, sm.act_dist, na);
            wave_sync();
            const uint32_t bits = lane < na ? sm.act_dist[lane] : kNanBits;
            const bool ok = lane < na && range_within(lim, q, bits);
            const uint64_t m = __ballot(ok);
            if (keys && ok) keys[dst + taken + (uint32_t)__popcll(m & below)] = ((uint64_t)bits << 32) | id;
            taken += (uint32_t)__popcll(m);
            wave_sync();
        }
        if (!keys && lane == 0) seg_cnt[w] = taken;
    }
}

// seg_off [np * S + 1]: the prefix sum over the first run's counts.  Pending row p is closed: count, offset, rung EXACT; ex_off /
// ex_len [np]: where the sort finds its keys.
__global__ void range_close_kernel(RangeState st, const uint32_t* __restrict__ list, uint32_t np, uint32_t S,
                                   const uint64_t* __restrict__ seg_off, uint64_t* __restrict__ ex_off, uint32_t* __restrict__ ex_len) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
    for (size_t p = tid; p < np; p += nth) {
        const uint32_t q = list ? list[p] : (uint32_t)p;
        const uint64_t a = seg_off[p * S], b = seg_off[(p + 1u) * S];
        st.count[q] = (uint32_t)(b - a);
        st.off[q] = a;
        st.rung[q] = kRungExact;
        st.pending[q] = 0u;
        ex_off[p] = a;
        ex_len[p] = (uint32_t)(b - a);
    }
}

// ---- the sort ----------------------------------------------------------------------------------------------------------------------
// List p: keys + ex_off[p], ex_len[p] keys, all distinct.  The network over the padded length (a power of two) with ascending
// comparators only: for k = 2, 4, ...: flip(k): i <-> (i | (k - 1)) - (i & (k / 2 - 1)) ... written below as block * k + k - 1 - r;
// then disperse(j) for j = k / 4 ... 1: i <-> i + j.  A comparator whose upper end is >= the length would compare with +infinity
// padding and never swaps: it is skipped, so no padding exists in memory.  A list shorter than the batch's longest is sorted after
// its own last level; the later levels find it sorted and swap nothing.
enum : uint32_t { kSortLocal = 0u, kSortLocalTail = 1u, kSortFlip = 2u, kSortDisperse = 3u };

__device__ __forceinline__ void range_cmpx(uint64_t* a, uint32_t i, uint32_t j) {
    const uint64_t x = a[i], y = a[j];
    if (x > y) { a[i] = y; a[j] = x; }
}

// chunk: a power of two >= 128, chunk * 8 bytes of dynamic LDS.  chunks_max / pairs_max: chunks, comparators (half the padded length) of
// the longest list.  kSortLocal: every chunk sorted (levels 2 ... chunk).  kSortLocalTail: disperse(chunk / 2 ... 1) of every chunk.
// kSortFlip / kSortDisperse: ONE stride of level k in global memory, a comparator per lane.
__global__ __launch_bounds__(64) void range_sort_kernel(uint64_t* __restrict__ keys, const uint64_t* __restrict__ ex_off,
                                                        const uint32_t* __restrict__ ex_len, uint32_t np, uint32_t chunk,
                                                        uint32_t chunks_max, uint64_t pairs_max, uint32_t mode, uint64_t k, uint64_t j) {
    const int lane = lane_id();
    if (mode == kSortLocal || mode == kSortLocalTail) {
        IDIST_DYN_SMEM(smem_raw);
        uint64_t* a = reinterpret_cast<uint64_t*>(smem_raw);
        const uint64_t items = (uint64_t)np * chunks_max;
        const uint32_t half = chunk / 2u;
        for (uint64_t w = blockIdx.x; w < items; w += gridDim.x) {
            const uint32_t p = (uint32_t)(w / chunks_max);
            const uint64_t start = (w % chunks_max) * chunk;
            const uint64_t len = ex_len[p];
            if (start >= len) continue;
            uint64_t* src = keys + ex_off[p] + start;
            const uint32_t have = len - start < chunk ? (uint32_t)(len - start) : chunk;
            wave_sync();
            for (uint32_t i = (uint32_t)lane; i < chunk; i += 64u) a[i] = i < have ? src[i] : ~0ull;
            wave_sync();
            for (uint32_t kk = mode == kSortLocal ? 2u : chunk; kk <= chunk; kk <<= 1) {
                if (mode == kSortLocal) {
                    const uint32_t hk = kk / 2u;
                    for (uint32_t t = (uint32_t)lane; t < half; t += 64u) {
                        const uint32_t blk = t / hk, r = t % hk;
                        range_cmpx(a, blk * kk + r, blk * kk + kk - 1u - r);
                    }
                    wave_sync();
                }
                for (uint32_t jj = mode == kSortLocal ? kk / 4u : half; jj >= 1u; jj >>= 1) {
                    for (uint32_t t = (uint32_t)lane; t < half; t += 64u) {
                        const uint32_t i = (t / jj) * 2u * jj + t % jj;
                        range_cmpx(a, i, i + jj);
                    }
                    wave_sync();
                }
            }
            for (uint32_t i = (uint32_t)lane; i < have; i += 64u) src[i] = a[i];
        }
        return;
    }
    const uint64_t waves = (pairs_max + 63u) / 64u, items = (uint64_t)np * waves;
    for (uint64_t w = blockIdx.x; w < items; w += gridDim.x) {
        const uint32_t p = (uint32_t)(w / waves);
        const uint64_t t = (w % waves) * 64u + (uint64_t)lane;
        const uint64_t len = ex_len[p];
        uint64_t i, o;
        if (mode == kSortFlip) {
            const uint64_t hk = k / 2u, blk = t / hk, r = t % hk;
            i = blk * k + r;
            o = blk * k + k - 1u - r;
        } else {
            i = (t / j) * 2u * j + t % j;
            o = i + j;
        }
        if (t < pairs_max && o < len) {
            uint64_t* a = keys + ex_off[p];
            const uint64_t x = a[i], y = a[o];
            if (x > y) { a[i] = y; a[o] = x; }
        }
    }
}

// lims [nq + 1]: the prefix sum of st.count.  out_pid / out_dist [lims[nq]].
__global__ __launch_bounds__(64) void range_gather_kernel(RangeState st, const uint64_t* __restrict__ keys, const uint64_t* __restrict__ lims,
                                                          uint32_t metric, uint32_t* __restrict__ out_pid, float* __restrict__ out_dist) {
    const int lane = lane_id();
    for (uint32_t q = blockIdx.x; q < st.nq; q += gridDim.x) {
        const uint64_t* src = keys + st.off[q];
        const uint64_t dst = lims[q];
        const uint32_t c = st.count[q];
        const float t = st.term[q];
        for (uint32_t i = (uint32_t)lane; i < c; i += 64u) {
            const uint64_t key = src[i];
            out_pid[dst + i] = (uint32_t)key;
            out_dist[dst + i] = range_report(metric, __uint_as_float((uint32_t)(key >> 32)), t);
        }
    }
}

}  // namespace idist
