// idist_grouped.hpp — the kernels of the grouped search (idist_search_batch_grouped, include/idist.h): the nearest
// allowed point of each of the k nearest groups, the group of point i being one u32 column of an attribute table, g(i).
//
// The search is the several-sets ladder of idist_allowed.hpp with ONE step exchanged: where allowed_select_kernel keeps the first k
// allowed entries of a list, grouped_select_kernel keeps the first k allowed entries that OPEN a group —
//
//   collapse(L): walk L in order; keep an entry iff it is allowed and no earlier kept entry has its group; stop after k.
//
//   grouped_select_kernel   one wave per list, 64 entries per step.  A lane loads its id, tests the bit of the query's own bitmap and
//                           gathers g(id).  The groups seen so far live in a set in LDS, one 64-bit slot per group:
//                           (list position + 1) << 32 | group, 0 = empty — every u32 is a legal group, so occupancy is the high word,
//                           never a reserved value.  A lane inserts (position + 1, group) with a 64-bit compare-and-swap and, where the
//                           group is there already, lowers the slot's position to its own if that is smaller: whatever the order in
//                           which the lanes of a step get to a slot, it ends up holding the SMALLEST list position of its group.  After
//                           the step's barrier a lane keeps its entry iff the slot holds its own position — the first allowed
//                           occurrence in list order, within the step and across steps — and the output position comes from a ballot
//                           over the keepers and a prefix popcount.  Which lane won an empty slot decides nothing.  The loop ends once k
//                           are kept.  The set has max(256, the power of two >= 2k) slots: at most k - 1 + 64 groups are ever in it.
//                           Three modes: a rung (the query is closed iff k were kept; the rung's counters are added either way), a
//                           round of the exact step (the kept entries are appended behind the query's count; closed when the count
//                           reaches k or the round's list was shorter than its width), and the kernel on its own (row q = collapse of
//                           list q, padded, every output word written once).
//   grouped_exclude_kernel  the bitmaps of an exact round: for pending row p of query q, A(q) AND "g(i) is none of the groups found for
//                           q so far".  The found groups (<= k) go into the same kind of set; a wave takes 64 points per step, one
//                           ballot gives two output words.  Every word written exactly once, the bits at positions >= n zero; windows
//                           without an allowed point cost one load.
//
// No global atomics; nothing but ballots, popcounts, LDS compare-and-swap and wave barriers.
#pragma once
#include "idist_allowed.hpp"

namespace idist {

enum : uint32_t { kGroupedRung = 0u, kGroupedRound = 1u, kGroupedWhole = 2u };

struct GroupedOut {
    uint32_t* pid;        // [nq][k]
    uint32_t* dist;       // [nq][k] f32 bit patterns
    uint32_t* group;      // [nq][k]
    uint32_t* count;      // [nq]
    uint32_t* rung;       // [nq]     (not in kGroupedWhole)
    uint32_t* counters;   // [nq][3] or nullptr
    uint32_t* pending;    // [nq]     (not in kGroupedWhole)
    uint32_t k;
};

// log2 of the slots of the set of seen groups: a power of two >= 2k, at least 256 — k <= 4096: at most 8192 slots, 64 KiB
__host__ __device__ inline uint32_t grouped_tab_log2(uint32_t k) {
    uint32_t l = 8u;
    while ((1u << l) < 2u * k) l++;
    return l;
}

__device__ __forceinline__ uint32_t grouped_hash(uint32_t g, uint32_t shift) { return (g * 0x9E3779B1u) >> shift; }

// (stamp, g) into the set: the slot of g, which afterwards holds min(stamp, what it held).  stamp >= 1.  The set is never full.
__device__ __forceinline__ uint32_t grouped_insert(unsigned long long* tab, uint32_t mask, uint32_t shift, uint32_t g, uint32_t stamp) {
    const unsigned long long mine = ((unsigned long long)stamp << 32) | g;
    uint32_t s = grouped_hash(g, shift);
    for (;;) {
        unsigned long long old = atomicCAS(&tab[s], 0ull, mine);
        if (old == 0ull) return s;
        if ((uint32_t)old == g) {
            while ((uint32_t)(old >> 32) > stamp) {
                const unsigned long long prev = atomicCAS(&tab[s], old, mine);
                if (prev == old) break;
                old = prev;
            }
            return s;
        }
        s = (s + 1u) & mask;
    }
}

__device__ __forceinline__ bool grouped_contains(const unsigned long long* tab, uint32_t mask, uint32_t shift, uint32_t g) {
    for (uint32_t s = grouped_hash(g, shift);; s = (s + 1u) & mask) {
        const unsigned long long v = tab[s];
        if (v == 0ull) return false;
        if ((uint32_t)v == g) return true;
    }
}

__device__ __forceinline__ void grouped_clear(unsigned long long* tab, uint32_t slots) {
    wave_sync();
    for (uint32_t s = (uint32_t)lane_id(); s < slots; s += 64u) tab[s] = 0ull;
    wave_sync();
}

// r_pid / r_dist [np][width], r_count [np], r_counters [np][3] or nullptr: the lists; list [np] (nullptr: the identity): the query q
// of list p.  groups [n]: g.  bits (nullptr: every id < n is allowed): query q reads the bitmap at bits + (set_of ? set_of[q] : q) *
// words.  Of a list only the first min(count, width) entries are read; an id >= n is not allowed and never dereferenced.
// Dynamic LDS: 8 << tab_log2 bytes, tab_log2 = grouped_tab_log2(o.k).
__global__ __launch_bounds__(64) void grouped_select_kernel(GroupedOut o, const uint32_t* __restrict__ groups, uint32_t n,
                                                            const uint32_t* __restrict__ bits, uint32_t words,
                                                            const uint32_t* __restrict__ set_of, const uint32_t* __restrict__ r_pid,
                                                            const uint32_t* __restrict__ r_dist, const uint32_t* __restrict__ r_count,
                                                            const uint32_t* __restrict__ r_counters, uint32_t width,
                                                            const uint32_t* __restrict__ list, uint32_t np, uint32_t rung, uint32_t mode,
                                                            uint32_t tab_log2) {
    IDIST_DYN_SMEM(smem_raw);
    unsigned long long* tab = reinterpret_cast<unsigned long long*>(smem_raw);
    const uint32_t slots = 1u << tab_log2, smask = slots - 1u, shift = 32u - tab_log2;
    const int lane = lane_id();
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint32_t p = blockIdx.x; p < np; p += gridDim.x) {
        const uint32_t q = list ? list[p] : p;
        const uint32_t* b = bits ? bits + (size_t)(set_of ? set_of[q] : q) * words : nullptr;
        uint32_t cnt = r_count[p];
        cnt = cnt < width ? cnt : width;
        const uint32_t base = mode == kGroupedRound ? o.count[q] : 0u;      // < k: the query is pending
        const uint32_t limit = o.k - base;
        const uint32_t* row_pid = r_pid + (size_t)p * width;
        const uint32_t* row_dist = r_dist + (size_t)p * width;
        uint32_t* o_pid = o.pid + (size_t)q * o.k;
        uint32_t* o_dist = o.dist + (size_t)q * o.k;
        uint32_t* o_group = o.group + (size_t)q * o.k;
        grouped_clear(tab, slots);
        uint32_t taken = 0;
        for (uint32_t i0 = 0; i0 < cnt && taken < limit; i0 += 64u) {
            const uint32_t i = i0 + (uint32_t)lane;
            uint32_t id = kInvalid;
            if (i < cnt) id = row_pid[i];
            // (the group does not wait for the bit: both gathers are in flight together)
            const bool in = i < cnt && id < n;
            uint32_t g = 0u, word = 0xFFFFFFFFu, slot = 0u;
            if (in) {
                g = groups[id];
                if (b) word = b[id >> 5];
            }
            const bool ok = in && ((word >> (id & 31u)) & 1u) != 0u;
            if (ok) slot = grouped_insert(tab, smask, shift, g, i + 1u);
            wave_sync();
            const bool keep = ok && (uint32_t)(tab[slot] >> 32) == i + 1u;   // the first allowed entry of its group, in list order
            const uint64_t m = __ballot(keep);
            const uint32_t pos = taken + (uint32_t)__popcll(m & below);
            if (keep && pos < limit) {
                o_pid[base + pos] = id;
                o_dist[base + pos] = row_dist[i];
                o_group[base + pos] = g;
            }
            taken += (uint32_t)__popcll(m);
        }
        taken = taken < limit ? taken : limit;
        const uint32_t total = base + taken;
        if (o.counters && r_counters && lane < 3) o.counters[(size_t)q * 3u + lane] += r_counters[(size_t)p * 3u + lane];
        const bool close = mode == kGroupedWhole || total == o.k || (mode == kGroupedRound && cnt < width);
        if (close) {
            for (uint32_t r = total + (uint32_t)lane; r < o.k; r += 64u) {
                o_pid[r] = kInvalid;
                o_dist[r] = 0x7f800000u;
                o_group[r] = 0u;
            }
        }
        if (lane == 0) {
            if (close || mode == kGroupedRound) o.count[q] = total;
            if (close && mode != kGroupedWhole) {
                o.rung[q] = rung;
                o.pending[q] = 0u;
            }
        }
    }
}

// The bitmaps of an exact round.  bits [n_sets][words] (nullptr: every point is allowed), set_of [nq], list [np] (nullptr: the
// identity) as allowed_scan_bits_kernel reads them; found [nq][k] / count [nq]: the groups found for a query so far.  out [np][words]: bit i of row p = bit i of the
// query's set (i < n) and g(i) not among its found groups.  The ceil(n / 64) windows of a row are cut into S contiguous segments, work
// item w = p * S + s; ident [np] = 0, 1, ... (what the scan takes as set_of for these rows).  Dynamic LDS as grouped_select_kernel.
__global__ __launch_bounds__(64) void grouped_exclude_kernel(const uint32_t* __restrict__ bits, uint32_t n, uint32_t words,
                                                             const uint32_t* __restrict__ set_of, const uint32_t* __restrict__ list,
                                                             uint32_t np, const uint32_t* __restrict__ groups,
                                                             const uint32_t* __restrict__ found, const uint32_t* __restrict__ count,
                                                             uint32_t k, uint32_t S, uint32_t tab_log2, uint32_t* __restrict__ out,
                                                             uint32_t* __restrict__ ident) {
    IDIST_DYN_SMEM(smem_raw);
    unsigned long long* tab = reinterpret_cast<unsigned long long*>(smem_raw);
    const uint32_t slots = 1u << tab_log2, smask = slots - 1u, shift = 32u - tab_log2;
    const int lane = lane_id();
    const uint32_t n_win = (uint32_t)(((uint64_t)n + 63u) / 64u);
    const uint64_t items = (uint64_t)np * S;
    for (uint64_t w = blockIdx.x; w < items; w += gridDim.x) {
        uint32_t p, lo, hi;
        scan_segment(n_win, S, w, &p, &lo, &hi);
        const uint32_t q = list ? list[p] : p;
        const uint32_t* b = bits ? bits + (size_t)set_of[q] * words : nullptr;
        uint32_t c = count[q];
        c = c < k ? c : k;
        grouped_clear(tab, slots);
        for (uint32_t j = (uint32_t)lane; j < c; j += 64u) grouped_insert(tab, smask, shift, found[(size_t)q * k + j], 1u);
        wave_sync();
        uint32_t* row = out + (size_t)p * words;
        for (uint32_t win = lo; win < hi; win++) {
            uint64_t m = ~0ull;                                          // (wave-uniform; the bits at positions >= n cleared)
            if (b) m = allowed_window(b, n, words, win);
            else if (64ull * win + 64u > n) m = (1ull << (n - 64ull * win)) - 1ull;
            if (m != 0ull && c != 0u) {
                bool on = ((m >> lane) & 1ull) != 0ull;
                if (on) on = !grouped_contains(tab, smask, shift, groups[64u * win + (uint32_t)lane]);
                m = __ballot(on);
            }
            const uint32_t wd = 2u * win + (uint32_t)lane;
            if (lane < 2 && wd < words) row[wd] = lane ? (uint32_t)(m >> 32) : (uint32_t)m;
        }
        if (w % S == 0u && lane == 0) ident[p] = p;
    }
}

}  // namespace idist
