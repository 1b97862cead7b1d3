// idist_attr.hpp — attribute filters: the allowed sets of a restricted search made ON the device (idist_search_batch_attr and its
// siblings, include/idist.h), and attribute tables: several columns, an OR of ANDs of interval clauses per query
// (idist_search_batch_match and its siblings; attr_match_kernel at the end of this file).
//
// The caller holds one u32 per point (a tenant id, a category, a day number) and one interval per query.  The values live on the
// device next to the rows (idist_attr); a call groups its distinct intervals on the host (at most nq of them), and this kernel
// turns them into the bitmaps every restricted search already reads:
//
//   attr_bitmaps_kernel    v [n], lo / hi [n_sets] -> out [n_sets][ceil(n / 32)]: bit i of out[s] = lo[s] <= v[i] && v[i] <= hi[s],
//                          UNSIGNED comparisons, i < n; the bits at positions >= n of a row's last word are written as 0.
//
// A wave owns a TILE of 64 windows of 64 points: lane j loads element j of every window (64 coalesced loads of 256 B, the 4096
// values stay in 64 VGPRs), and for every set the ballot of window w — a wave-uniform 64-bit mask — is kept by lane w.  Lane j then
// holds window j of the set's tile and stores its two u32 words: the wave writes the tile's 512 B of a row as two store
// instructions over one contiguous range.  u32 stores, because a row has ceil(n / 32) words: when that is odd every other row
// starts on an address that is no multiple of 8.  The second word of the last window is written only if the row has it (it would be
// the first word of the next row otherwise).  Work item = (tile, chunk of set_chunk sets); the grid strides over the items, every
// output word belongs to exactly one item and is written exactly once: no atomics, no memset in front, the same bytes whatever
// the grid and whatever set_chunk.  v is read once per chunk of sets (once in all when set_chunk >= n_sets).  No LDS.
#pragma once
#include "idist_kernels.hpp"

namespace idist {

constexpr uint32_t kAttrTile = 4096u;                    // points of a tile: 64 windows of 64

// lo[s] > hi[s] is the empty set.  Nothing is read past v[n - 1], nothing is written past a row's last word.  n >= 1, n_sets >= 1,
// set_chunk >= 1.
__global__ __launch_bounds__(64) void attr_bitmaps_kernel(const uint32_t* __restrict__ v, uint32_t n, const uint32_t* __restrict__ lo,
                                                          const uint32_t* __restrict__ hi, uint32_t n_sets, uint32_t set_chunk,
                                                          uint32_t* __restrict__ out) {
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t words = (uint32_t)(((uint64_t)n + 31u) / 32u);
    const uint32_t n_tiles = (uint32_t)(((uint64_t)n + kAttrTile - 1u) / kAttrTile);
    const uint32_t n_chunks = (n_sets + set_chunk - 1u) / set_chunk;
    const uint64_t items = (uint64_t)n_tiles * n_chunks;
    for (uint64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const uint32_t tile = (uint32_t)(it / n_chunks), chunk = (uint32_t)(it % n_chunks);
        const uint64_t base = (uint64_t)tile * kAttrTile;
        const uint32_t rem = n - base < kAttrTile ? (uint32_t)(n - base) : kAttrTile;     // points of this tile, 1..4096
        uint32_t x[64];                                       // x[w]: element `lane` of window w (0 beyond the tile: masked below)
#pragma unroll
        for (uint32_t w = 0; w < 64u; w++) {
            const uint32_t i = w * 64u + lane;
            x[w] = i < rem ? v[base + i] : 0u;
        }
        // the window this lane ends up holding: its valid bits, and where its words go
        const uint32_t have = rem > 64u * lane ? rem - 64u * lane : 0u;
        const uint64_t valid = have >= 64u ? ~0ull : (1ull << have) - 1ull;
        const uint64_t w0 = (uint64_t)tile * (kAttrTile / 32u) + 2u * lane;
        const uint32_t s_end = n_sets - chunk * set_chunk < set_chunk ? n_sets : (chunk + 1u) * set_chunk;
        for (uint32_t s = chunk * set_chunk; s < s_end; s++) {
            const uint32_t l = lo[s], h = hi[s];              // wave-uniform
            uint64_t m = 0;
#pragma unroll
            for (uint32_t w = 0; w < 64u; w++) {
                const uint64_t b = __ballot(l <= x[w] && x[w] <= h);
                if (lane == w) m = b;
            }
            m &= valid;
            uint32_t* row = out + (size_t)s * words;
            if (w0 < words) row[w0] = (uint32_t)m;
            if (w0 + 1u < words) row[w0 + 1u] = (uint32_t)(m >> 32);
        }
    }
}

// ---- attribute tables: several columns, AND / OR conditions (idist_search_batch_match and its siblings) ----
//
//   attr_match_kernel      v [n_cols][col_pitch], a program of n_sets conditions -> out [n_sets][ceil(n / 32)]:
//                          bit i of out[s] = OR over the conjunctions j in [or_lims[s], or_lims[s + 1]) of
//                                            AND over the clauses c in [and_lims[j], and_lims[j + 1]) of
//                                            lo_c <= v[col_c][i] && v[col_c][i] <= hi_c,       UNSIGNED, i < n
//                          (no conjunction: FALSE; a conjunction of no clause: TRUE); the bits at positions >= n are written as 0.
//
// The tile, the ownership of the windows and the two stores per lane are attr_bitmaps_kernel's, and so is its contract: every word
// written exactly once, the same bytes whatever the grid and set_chunk, no column read past its element n - 1, no LDS.  Per clause
// the 64 ballots of its column's tile are selected into the lanes that own the windows; the lane ANDs them into its conjunction's
// mask and ORs that into its condition's mask.  The program is read through wave-uniform addresses (scalar loads), and the loaded
// tile is KEPT while consecutive clauses — of one conjunction, of the next one, of the next condition — name the same column: a
// wave-uniform test.  The host orders the clauses of a conjunction by column, so a conjunction loads every column it names once.
struct AttrClause {
    uint32_t col, lo, hi;
};

// n >= 1, n_sets >= 1, set_chunk >= 1, col_pitch >= n.  A clause whose col >= n_cols reads nothing and matches nothing (the calls
// of include/idist.h refuse it before they launch).
__global__ __launch_bounds__(64) void attr_match_kernel(const uint32_t* __restrict__ v, uint32_t n, uint32_t n_cols, uint64_t col_pitch,
                                                        const AttrClause* __restrict__ clauses, const uint32_t* __restrict__ and_lims,
                                                        const uint32_t* __restrict__ or_lims, uint32_t n_sets, uint32_t set_chunk,
                                                        uint32_t* __restrict__ out) {
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t words = (uint32_t)(((uint64_t)n + 31u) / 32u);
    const uint32_t n_tiles = (uint32_t)(((uint64_t)n + kAttrTile - 1u) / kAttrTile);
    const uint32_t n_chunks = (n_sets + set_chunk - 1u) / set_chunk;
    const uint64_t items = (uint64_t)n_tiles * n_chunks;
    for (uint64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const uint32_t tile = (uint32_t)(it / n_chunks), chunk = (uint32_t)(it % n_chunks);
        const uint64_t base = (uint64_t)tile * kAttrTile;
        const uint32_t rem = n - base < kAttrTile ? (uint32_t)(n - base) : kAttrTile;     // points of this tile, 1..4096
        uint32_t x[64];                                       // x[w]: element `lane` of window w of column `held` (0 beyond the tile)
        uint32_t held = 0xFFFFFFFFu;                          // wave-uniform: the column x holds (none yet)
#pragma unroll
        for (uint32_t w = 0; w < 64u; w++) x[w] = 0u;
        const uint32_t have = rem > 64u * lane ? rem - 64u * lane : 0u;
        const uint64_t valid = have >= 64u ? ~0ull : (1ull << have) - 1ull;
        const uint64_t w0 = (uint64_t)tile * (kAttrTile / 32u) + 2u * lane;
        const uint32_t s_end = n_sets - chunk * set_chunk < set_chunk ? n_sets : (chunk + 1u) * set_chunk;
        for (uint32_t s = chunk * set_chunk; s < s_end; s++) {
            uint64_t cond = 0;                                // window `lane` of condition s
            const uint32_t j_end = or_lims[s + 1u];
            for (uint32_t j = or_lims[s]; j < j_end; j++) {
                uint64_t conj = ~0ull;
                const uint32_t c_end = and_lims[j + 1u];
                for (uint32_t c = and_lims[j]; c < c_end; c++) {
                    const uint32_t col = clauses[c].col, l = clauses[c].lo, h = clauses[c].hi;   // wave-uniform
                    if (col >= n_cols) {
                        conj = 0;
                        continue;
                    }
                    if (col != held) {
                        const uint32_t* vc = v + (uint64_t)col * col_pitch + base;
#pragma unroll
                        for (uint32_t w = 0; w < 64u; w++) {
                            const uint32_t i = w * 64u + lane;
                            x[w] = i < rem ? vc[i] : 0u;
                        }
                        held = col;
                    }
                    uint64_t m = 0;
#pragma unroll
                    for (uint32_t w = 0; w < 64u; w++) {
                        const uint64_t b = __ballot(l <= x[w] && x[w] <= h);
                        if (lane == w) m = b;
                    }
                    conj &= m;
                }
                cond |= conj;
            }
            cond &= valid;
            uint32_t* row = out + (size_t)s * words;
            if (w0 < words) row[w0] = (uint32_t)cond;
            if (w0 + 1u < words) row[w0 + 1u] = (uint32_t)(cond >> 32);
        }
    }
}

}  // namespace idist
