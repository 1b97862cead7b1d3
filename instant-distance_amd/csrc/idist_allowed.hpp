// idist_allowed.hpp — the kernels around a restricted search (idist_search_batch_allowed, include/idist.h).
//
// A restricted search is DEFINED through what is already bit-exact: Hnsw::search at growing ef_search (the "rungs"), filtered by
// the allowed set A, and an exact scan of A's rows where the ladder does not apply or ends.  The walk kernels are not touched;
// everything here runs between their launches, on the launch's stream:
//
//   allowed_init_kernel     the result rows of all nq queries padded (kInvalid / +inf), count 0, rung NONE, counters 0, every query
//                           pending.
//   allowed_select_kernel   one wave per pending query: its rung result row against the bitmap (n / 8 bytes, L2-resident), ballot +
//                           prefix-popcount compaction of the first k allowed entries into the row of the ORIGINAL query index.  k
//                           found: count, rung, no longer pending.  The counters of the rung are added either way.  The same
//                           kernel finishes the exact step (every entry of the merged scan is allowed): it writes what there is,
//                           pads the row and closes the query whatever the count.
//   allowed_pending_kernel  the pending queries in ascending order (a wave per 64 queries: the set flags in front of its chunk are
//                           counted, not scanned — no atomics, the same list whatever the schedule), and their prepared rows
//                           gathered into a contiguous buffer for the next rung's launch.
//   allowed_scan_kernel     the exact step: the shared steps of the exact scans (scan_segment, stage_query, scan_rank_batch with
//                           ef = k, topk_emit_list: idist_device.hpp / idist_kernels.hpp) over one contiguous segment of the
//                           ascending id list of A per wave; grid = pending queries x S segments.  Each
//                           wave writes its segment's sorted top-k as list s in merge_topk_kernel's input layout (base 0): the
//                           merge by (distance bits, id) gives the k best, and ids are distinct, so the result does not depend on S.
//
// Several allowed sets per call, one per query (idist_search_batch_allowed_sets): row q is what the single-set call returns for
// query q alone with its own set, so the same kernels serve, told which bitmap a query reads:
//
//   allowed_count_kernel      one wave per set: popcount of its words (the last partial word masked), then the start rule
//                             E[r] * |A| >= k * n in 64-bit integers -> start[s]: a rung index, kRungExact (|A| <= k, or no permitted
//                             rung qualifies) or kRungNone (the empty set).  No atomics.
//   allowed_init_kernel       with a start table: first[q] = start[set of q]; a query whose set is empty is closed at once.
//   allowed_select_kernel     with set_of: the row is filtered by the bitmap of the query's own set.
//   allowed_pending_kernel    with first / rung: a query is gathered iff it is pending and first[q] <= rung — a query waits,
//                             unlaunched, until its start rung comes up; rung = kRungExact gathers everything still pending.
//                             With last (the restricted range search, idist_range_allowed.hpp): ... and rung < last[q].
//   allowed_scan_bits_kernel  the exact step straight from the bitmap: grid = pending queries x S segments of the 64-id windows of
//                             [0, n).  A wave takes 64 windows at a time (one 64-bit load per lane), skips the all-zero ones by a
//                             ballot, and compacts the set bits of the others into ascending ids by prefix popcount, in batches of
//                             64 in act_pid; an id that does not fit the batch stays in its lane's register until the batch has been
//                             ranked (scan_rank_batch) and opens the next one.  Staging and output are allowed_scan_kernel's.  No id
//                             list exists, on the host or the device; the staging does not depend on the number of sets.
//
// The partitioned index (idist_partitioned_search_batch_allowed_sets): every part runs the several-sets call on ITS slice of the
// caller's global bitmaps, and base[p] is no multiple of 32 in general:
//
//   allowed_slice_kernel      out[s] bit i = in[s] bit bit_offset + i, i < n_out: one lane per output word, two adjacent source words
//                             joined by a 64-bit shift, the last word of a row masked.  No LDS, no atomics.
#pragma once
#include "idist_kernels.hpp"
#include "idist_merge.hpp"

namespace idist {

constexpr uint32_t kRungNone = 254u;     // IDIST_RUNG_NONE
constexpr uint32_t kRungExact = 255u;    // IDIST_RUNG_EXACT

__device__ __forceinline__ bool allowed_bit(const uint32_t* __restrict__ bits, uint32_t n, uint32_t pid) {
    return pid < n && ((bits[pid >> 5] >> (pid & 31u)) & 1u) != 0u;
}

struct AllowedOut {
    uint32_t* pid;        // [nq][k]
    uint32_t* dist;       // [nq][k] f32 bit patterns
    uint32_t* count;      // [nq]
    uint32_t* rung;       // [nq]
    uint32_t* counters;   // [nq][3] or nullptr
    uint32_t* pending;    // [nq] 1: not answered yet
    uint32_t nq, k;
};

// start [n_sets] / set_of [nq] / first [nq]: the several-sets call (start == nullptr: one set, every query pending).  first[q] =
// start[set_of[q]]: the first rung query q runs, kRungExact, or kRungNone — the query is then closed here, with count 0.
__global__ void allowed_init_kernel(AllowedOut o, const uint32_t* __restrict__ start = nullptr, const uint32_t* __restrict__ set_of = nullptr,
                                    uint32_t* __restrict__ first = nullptr) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
    const size_t total = (size_t)o.nq * o.k;
    for (size_t i = tid; i < total; i += nth) {
        o.pid[i] = kInvalid;
        o.dist[i] = 0x7f800000u;
    }
    for (size_t q = tid; q < o.nq; q += nth) {
        o.count[q] = 0u;
        o.rung[q] = kRungNone;
        uint32_t f = 0u;
        if (start) {
            f = start[set_of[q]];
            first[q] = f;
        }
        o.pending[q] = f == kRungNone ? 0u : 1u;
        if (o.counters) { o.counters[3 * q] = 0u; o.counters[3 * q + 1] = 0u; o.counters[3 * q + 2] = 0u; }
    }
}

// r_pid / r_dist: [np][width] result rows of the np pending queries, r_count [np], r_counters [np][3] or nullptr.  list [np]: the
// original query index of every row (nullptr: the identity).  rung: what a query answered here reports.  exact != 0: the rows are
// the merged scan of A — written, padded and closed whatever their count.  set_of [nq] (nullptr: one set): query q reads the bitmap
// at bits + set_of[q] * words.
__global__ __launch_bounds__(64) void allowed_select_kernel(AllowedOut o, const uint32_t* __restrict__ bits, uint32_t n,
                                                            const uint32_t* __restrict__ r_pid, const uint32_t* __restrict__ r_dist,
                                                            const uint32_t* __restrict__ r_count, const uint32_t* __restrict__ r_counters,
                                                            uint32_t width, const uint32_t* __restrict__ list, uint32_t np,
                                                            uint32_t rung, uint32_t exact,
                                                            const uint32_t* __restrict__ set_of = nullptr, uint32_t words = 0) {
    const int lane = lane_id();
    const uint64_t below = (1ull << lane) - 1ull;
    const uint32_t* const all_bits = bits;
    for (uint32_t p = blockIdx.x; p < np; p += gridDim.x) {
        const uint32_t q = list ? list[p] : p;
        if (set_of) bits = all_bits + (size_t)set_of[q] * words;
        uint32_t cnt = r_count[p];
        cnt = cnt < width ? cnt : width;
        const uint32_t* row_pid = r_pid + (size_t)p * width;
        const uint32_t* row_dist = r_dist + (size_t)p * width;
        uint32_t* o_pid = o.pid + (size_t)q * o.k;
        uint32_t* o_dist = o.dist + (size_t)q * o.k;
        uint32_t taken = 0;
        for (uint32_t i0 = 0; i0 < cnt && taken < o.k; i0 += 64u) {
            const uint32_t i = i0 + (uint32_t)lane;
            uint32_t id = kInvalid;
            if (i < cnt) id = row_pid[i];
            const bool ok = i < cnt && allowed_bit(bits, n, id);
            const uint64_t m = __ballot(ok);
            const uint32_t pos = taken + (uint32_t)__popcll(m & below);
            if (ok && pos < o.k) {
                o_pid[pos] = id;
                o_dist[pos] = row_dist[i];
            }
            taken += (uint32_t)__popcll(m);
        }
        taken = taken < o.k ? taken : o.k;
        if (o.counters && r_counters && lane < 3) o.counters[(size_t)q * 3u + lane] += r_counters[(size_t)p * 3u + lane];
        if (exact) {
            for (uint32_t r = taken + (uint32_t)lane; r < o.k; r += 64u) {
                o_pid[r] = kInvalid;
                o_dist[r] = 0x7f800000u;
            }
        }
        if (lane == 0 && (exact || taken == o.k)) {
            o.count[q] = taken;
            o.rung[q] = rung;
            o.pending[q] = 0u;
        }
    }
}

// pending [nq] -> list: the pending query indices, ascending; pend_q [np][kdim]: their rows of `queries` [nq][kdim]; *n_pending = np.
// grid = ceil(nq / 64) waves EXACTLY: wave b owns the queries [64 b, 64 b + 64) and the last one writes the total.
// first [nq] (nullptr: every pending query is gathered): only the pending queries with first[q] <= rung are — the others wait.
// last [nq] (nullptr: no bound; the restricted range search, idist_range_allowed.hpp): only those with rung < last[q] are — the
// others have run their last rung and wait for the exact step.
__global__ __launch_bounds__(64) void allowed_pending_kernel(const uint32_t* __restrict__ pending, uint32_t nq,
                                                             const float* __restrict__ queries, uint32_t kdim,
                                                             uint32_t* __restrict__ list, float* __restrict__ pend_q,
                                                             uint32_t* __restrict__ n_pending,
                                                             const uint32_t* __restrict__ first_rung = nullptr, uint32_t rung = 0,
                                                             const uint32_t* __restrict__ last_rung = nullptr) {
    const int lane = lane_id();
    const uint32_t first = blockIdx.x * 64u;
    auto due = [&](uint32_t i) { return pending[i] != 0u && (!first_rung || first_rung[i] <= rung) && (!last_rung || rung < last_rung[i]); };
    uint32_t before = 0;
    for (uint32_t i = (uint32_t)lane; i < first; i += 64u) before += due(i) ? 1u : 0u;
    before = wave_sum_u32(before);
    const uint32_t q = first + (uint32_t)lane;
    const bool on = q < nq && due(q);
    const uint64_t m = __ballot(on);
    if (on) list[before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = q;
    uint64_t rest = m;
    uint32_t pos = before;
    while (rest) {
        const int j = __builtin_ctzll(rest);
        rest &= rest - 1ull;
        const float* src = queries + (size_t)(first + (uint32_t)j) * kdim;
        float* dst = pend_q + (size_t)pos * kdim;
        for (uint32_t e = (uint32_t)lane; e < kdim; e += 64u) dst[e] = src[e];
        pos++;
    }
    if (blockIdx.x == gridDim.x - 1u && lane == 0) *n_pending = before + (uint32_t)__popcll(m);
}

// The exact step.  ids [n_ids]: A's points, ascending; cut into S contiguous segments [n_ids s / S, n_ids (s + 1) / S).  queries
// [np][dim]: the pending queries' rows.  Work item w = p * S + s; out_pid / out_dist [S][np][k], out_count [S][np] (merge_topk_kernel's
// input layout).  Only the first out_count entries of a list are written.
template <int NB, int RS, int TAIL>
__global__ __launch_bounds__(64) void allowed_scan_kernel(IndexView ix, const float* __restrict__ queries, uint32_t np,
                                                          const uint32_t* __restrict__ ids, uint32_t n_ids, uint32_t S, uint32_t k,
                                                          uint32_t wcap, uint32_t* out_pid, uint32_t* out_dist, uint32_t* out_count) {
    IDIST_DYN_SMEM(smem_raw);
    const Smem sm = carve(smem_raw, ix.stride, wcap, false);
    const int lane = lane_id();
    const uint64_t items = (uint64_t)np * S;
    for (uint64_t w = blockIdx.x; w < items; w += gridDim.x) {
        uint32_t p, lo, hi;
        scan_segment(n_ids, S, w, &p, &lo, &hi);
        stage_query<NB>(ix, sm.q, queries + (size_t)p * ix.dim);
        WState st{sm.W, 0, (int)k, 0, 0u};
        for (uint32_t base = lo; base < hi; base += 64u) {
            const int na = hi - base < 64u ? (int)(hi - base) : 64;
            if (lane < na) sm.act_pid[lane] = ids[base + (uint32_t)lane];
            scan_rank_batch<NB, RS, TAIL>(ix, sm, st, na);
        }
        const size_t slot = (size_t)(w % S) * np + p;
        topk_emit_list(st, slot * k, slot, out_pid, out_dist, out_count);
    }
}

// ---- several sets per call ----------------------------------------------------------------------------------------------------

struct AllowedLadder {
    uint32_t E[8];        // ef_search of the permitted rungs
    uint32_t n_rungs;     // (max_rungs applied)
};

// |A| of one bitmap of `words` words over n points (bits at positions >= n not counted), in every lane: a sum of popcounts, the same
// whatever the schedule.  <= n.
__device__ __forceinline__ uint32_t allowed_set_size(const uint32_t* __restrict__ b, uint32_t n, uint32_t words) {
    const uint32_t last_mask = n % 32u ? (1u << (n % 32u)) - 1u : 0xFFFFFFFFu;
    uint32_t c = 0;
    for (uint32_t w = (uint32_t)lane_id(); w < words; w += 64u) {
        const uint32_t v = b[w] & (w + 1u == words ? last_mask : 0xFFFFFFFFu);
        c += (uint32_t)__popcll((uint64_t)v);
    }
    return wave_sum_u32(c);
}

// bits [n_sets][words] -> size [n_sets] = |A_s| (bits at positions >= n not counted), start [n_sets]: the first permitted rung r
// with E[r] |A_s| >= k n (64-bit), kRungExact when |A_s| <= k or no rung qualifies, kRungNone for the empty set.  One wave per set
// (the grid strides over the rest): a sum of popcounts, the same whatever the schedule.
__global__ __launch_bounds__(64) void allowed_count_kernel(const uint32_t* __restrict__ bits, uint32_t n, uint32_t words, uint32_t n_sets,
                                                           uint32_t k, AllowedLadder lad, uint32_t* __restrict__ size,
                                                           uint32_t* __restrict__ start) {
    const int lane = lane_id();
    for (uint32_t s = blockIdx.x; s < n_sets; s += gridDim.x) {
        const uint32_t c = allowed_set_size(bits + (size_t)s * words, n, words);
        uint32_t r0 = kRungExact;
        if (c == 0u) r0 = kRungNone;
        else if (c > k)
            for (uint32_t r = 0; r < lad.n_rungs && r0 == kRungExact; r++)
                if ((uint64_t)lad.E[r] * c >= (uint64_t)k * n) r0 = r;
        if (lane == 0) {
            size[s] = c;
            start[s] = r0;
        }
    }
}

// The 64-bit window `win` (ids [64 win, 64 win + 64)) of a bitmap of `words` u32 words over n points, bits at positions >= n cleared.
__device__ __forceinline__ uint64_t allowed_window(const uint32_t* __restrict__ bits, uint32_t n, uint32_t words, uint32_t win) {
    const uint32_t w0 = 2u * win;
    uint64_t m = 0;
    if (w0 < words) m = bits[w0];
    if (w0 + 1u < words) m |= (uint64_t)bits[w0 + 1u] << 32;
    const uint64_t lo = 64ull * win;
    if (lo + 64u > n) m = lo >= n ? 0ull : m & ((1ull << (n - lo)) - 1ull);
    return m;
}

// The exact step of the several-sets call, straight from the bitmaps.  bits [n_sets][words]; list [np] (nullptr: the identity): the
// original query index of pending row p, set_of [nq]: its set.  The n_win = ceil(n / 64) windows of [0, n) are cut into S contiguous
// segments [n_win s / S, n_win (s + 1) / S) (an empty one yields an empty list).  Work item w = p * S + s; the outputs as
// allowed_scan_kernel's.  Ids reach act_pid ascending and are distinct, so the result depends neither on S nor on the batches.
template <int NB, int RS, int TAIL>
__global__ __launch_bounds__(64) void allowed_scan_bits_kernel(IndexView ix, const float* __restrict__ queries, uint32_t np,
                                                               const uint32_t* __restrict__ bits, uint32_t n, uint32_t words,
                                                               const uint32_t* __restrict__ list, const uint32_t* __restrict__ set_of,
                                                               uint32_t S, uint32_t k, uint32_t wcap, uint32_t* out_pid,
                                                               uint32_t* out_dist, uint32_t* out_count) {
    IDIST_DYN_SMEM(smem_raw);
    const Smem sm = carve(smem_raw, ix.stride, wcap, false);
    const int lane = lane_id();
    const uint64_t below = (1ull << lane) - 1ull;
    const uint32_t n_win = (uint32_t)(((uint64_t)n + 63u) / 64u);
    const uint64_t items = (uint64_t)np * S;
    for (uint64_t w = blockIdx.x; w < items; w += gridDim.x) {
        uint32_t p, lo, hi;
        scan_segment(n_win, S, w, &p, &lo, &hi);
        const uint32_t* b = bits + (size_t)set_of[list ? list[p] : p] * words;
        stage_query<NB>(ix, sm.q, queries + (size_t)p * ix.dim);
        WState st{sm.W, 0, (int)k, 0, 0u};
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
                const bool ok = ((m >> lane) & 1ull) != 0ull;
                const uint32_t id = (g + (uint32_t)j) * 64u + (uint32_t)lane;
                const uint32_t pos = fill + (uint32_t)__popcll(m & below);
                if (ok && pos < 64u) sm.act_pid[pos] = id;
                fill += (uint32_t)__popcll(m);
                if (fill >= 64u) {
                    scan_rank_batch<NB, RS, TAIL>(ix, sm, st, 64);
                    if (ok && pos >= 64u) sm.act_pid[pos - 64u] = id;     // carried over in the lane's register
                    fill -= 64u;
                }
            }
        }
        if (fill) scan_rank_batch<NB, RS, TAIL>(ix, sm, st, (int)fill);
        const size_t slot = (size_t)(w % S) * np + p;
        topk_emit_list(st, slot * k, slot, out_pid, out_dist, out_count);
    }
}

// ---- a bit range of every set: the slice of the global bitmaps that falls into one part ----------------------------------------------

// in [n_sets][pitch] words -> out [n_sets][ceil(n_out / 32)]: bit i of out[s] = bit bit_offset + i of in[s] for i < n_out, the bits
// at positions >= n_out of a row's last word 0.  Of a source row only the words below ceil((bit_offset + n_out) / 32) are read (the
// row may end there): the second word of a pair is loaded only when the shift needs it and it lies below that bound.  One lane per
// output word, consecutive lanes on consecutive words of a row; the grid strides over the rest.  n_out >= 1.
__global__ void allowed_slice_kernel(const uint32_t* __restrict__ in, uint32_t n_sets, uint32_t pitch, uint64_t bit_offset,
                                     uint32_t n_out, uint32_t* __restrict__ out) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
    const uint32_t words_out = (uint32_t)(((uint64_t)n_out + 31u) / 32u);
    const uint64_t w0 = bit_offset / 32u, w_end = (bit_offset + n_out + 31u) / 32u;
    const uint32_t sh = (uint32_t)(bit_offset % 32u);
    const uint32_t last_mask = n_out % 32u ? (1u << (n_out % 32u)) - 1u : 0xFFFFFFFFu;
    const size_t total = (size_t)n_sets * words_out;
    for (size_t i = tid; i < total; i += nth) {
        const size_t s = i / words_out;
        const uint32_t w = (uint32_t)(i % words_out);
        const uint32_t* row = in + s * pitch;
        const uint64_t a = w0 + w;                            // < w_end: bit 32 w of the slice exists
        uint64_t v = row[a];
        if (sh != 0u && a + 1u < w_end) v |= (uint64_t)row[a + 1u] << 32;
        uint32_t r = (uint32_t)(v >> sh);
        if (w + 1u == words_out) r &= last_mask;
        out[i] = r;
    }
}

}  // namespace idist
