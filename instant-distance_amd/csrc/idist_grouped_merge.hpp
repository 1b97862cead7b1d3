// idist_grouped_merge.hpp — the union step of the grouped search over a partitioned index (idist_partitioned_search_batch_grouped,
// idist_grouped_merge_device, include/idist.h): P collapsed lists per query -> the first k entries of their merged
// order that open a group.
//
// Every list is what the grouped search of one part returned: ascending in the key  distance bits << 32 | global id  and holding
// pairwise distinct groups.  The answer is collapse(merge of the lists): walk the merged order, keep an entry iff no earlier kept
// entry has its group, stop after k.  merge_topk_kernel cannot serve: a group may have members in several lists, so how far into the
// P * width entries the k-th distinct group lies is known only while walking.  So the kernel PRODUCES the merged order a tile at a
// time and stops when k are kept:
//
//   one wave per query, lane p owns list p's cursor, length, base and counters.  A step, with `a` lists not yet exhausted and
//   b = max(1, 64 / a): every active list proposes its next b entries (lane j: entry t = j % b of the (j / b)-th active list).
//   T = the minimum over the active lists of the LAST proposed key; a list that runs out inside its b proposals does not bound T.
//   Every unproposed key of a list exceeds that list's last proposal, which is >= T — so the proposals with key <= T are exactly the
//   next entries of the merged order (between b and 64 of them; all that is left when no list bounds T).  They are compacted into an
//   LDS tile by ballot and prefix popcount, each key is ranked inside the tile (the tile's keys are read as broadcasts), and the tile
//   is scattered into rank order.  Lane r then handles merged position seq + r: it inserts (seq + r + 1, group) into the set of seen
//   groups — grouped_select_kernel's set and its insert, idist_grouped.hpp: the smallest position of a group wins whatever the order
//   of the lanes — and keeps its entry iff the slot holds its own position.  Output position = kept so far + prefix popcount of the
//   keepers' ballot.  The cursors advance by what each list had taken (a popcount of its run of the ballot).
//
// LDS: the set, 8 B x max(256, pow2 >= 2k) — at most k - 1 + 64 groups are ever in it: every distinct group seen so far IS kept, and
// fewer than k were kept when a step starts — and 1792 B behind it (two 64-entry tiles of keys and groups, the active lists).  It
// does not grow with P or width; the lists are read where the parts wrote them.  A query whose groups rarely repeat across lists
// stops after about k entries; one whose lists all hold the same groups reads them all.  No size is refused, no global atomics,
// every output word is written exactly once, and the bytes do not depend on the grid.
#pragma once
#include "idist_grouped.hpp"
#include "idist_merge.hpp"

namespace idist {

constexpr uint32_t kGroupedMergeTileBytes = 64u * (8u + 8u + 4u + 4u + 4u);

struct GroupedMergeArgs {
    const uint32_t* pid;        // [n_lists][nq][width]
    const uint32_t* dist;       // [n_lists][nq][width] f32 bit patterns
    const uint32_t* group;      // [n_lists][nq][width]
    const uint32_t* count;      // [n_lists][nq]
    const uint32_t* counters;   // [n_lists][nq][3] or nullptr
    uint32_t n_lists, nq, width, k;
    uint32_t* out_pid;          // [nq][k]
    uint32_t* out_dist;         // [nq][k] f32 bit patterns
    uint32_t* out_group;        // [nq][k]
    uint32_t* out_count;        // [nq]
    uint32_t* out_counters;     // [nq][3] or nullptr
    uint32_t tab_log2;          // grouped_tab_log2(k)
    uint32_t base[kMergeMaxLists];
};

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

// Dynamic LDS: (8 << tab_log2) + kGroupedMergeTileBytes bytes.
__global__ __launch_bounds__(64) void grouped_merge_kernel(GroupedMergeArgs a) {
    IDIST_DYN_SMEM(smem_raw);
    unsigned long long* tab = reinterpret_cast<unsigned long long*>(smem_raw);
    const uint32_t slots = 1u << a.tab_log2, smask = slots - 1u, shift = 32u - a.tab_log2;
    uint64_t* tile_key = reinterpret_cast<uint64_t*>(smem_raw + ((size_t)8u << a.tab_log2));   // the step's entries, list after list
    uint64_t* sort_key = tile_key + 64;                                                        // ... in merged order
    uint32_t* tile_grp = reinterpret_cast<uint32_t*>(sort_key + 64);
    uint32_t* sort_grp = tile_grp + 64;
    uint32_t* act_s = sort_grp + 64;                                                           // the r-th active list
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t below = (1ull << lane) - 1ull;
    const uint32_t P = a.n_lists, nq = a.nq, w = a.width, k = a.k;
    const uint32_t base = lane < P ? a.base[lane] : 0u;
    for (uint32_t q = blockIdx.x; q < nq; q += gridDim.x) {
        uint32_t len = 0, c0 = 0, c1 = 0, c2 = 0;
        if (lane < P) {
            len = a.count[(size_t)lane * nq + q];
            len = len < w ? len : w;
            if (a.counters) {
                const uint32_t* s = a.counters + ((size_t)lane * nq + q) * 3u;
                c0 = s[0]; c1 = s[1]; c2 = s[2];
            }
        }
        uint32_t* o_pid = a.out_pid + (size_t)q * k;
        uint32_t* o_dist = a.out_dist + (size_t)q * k;
        uint32_t* o_group = a.out_group + (size_t)q * k;
        grouped_clear(tab, slots);
        uint32_t cur = 0, kept = 0, seq = 0;
        while (kept < k) {
            const bool active = cur < len;
            const uint64_t ma = __ballot(active);
            if (ma == 0ull) break;
            const uint32_t na = (uint32_t)__popcll(ma), b = 64u / na;
            const uint32_t mine = (uint32_t)__popcll(ma & below);            // an active list: its place among the active ones
            if (active) act_s[mine] = lane;
            wave_sync();
            // lane j proposes entry t of the r-th active list
            const uint32_t r = lane / b, t = lane - r * b;
            const bool prop = r < na;
            const uint32_t p = prop ? act_s[r] : 0u;
            const uint32_t i = (uint32_t)__shfl((int)cur, (int)p, 64) + t;
            const uint32_t p_len = (uint32_t)__shfl((int)len, (int)p, 64);
            const uint32_t p_base = (uint32_t)__shfl((int)base, (int)p, 64);
            const bool valid = prop && i < p_len;
            uint64_t key = ~0ull;
            uint32_t g = 0u;
            if (valid) {
                const size_t o = ((size_t)p * nq + q) * w + i;
                key = ((uint64_t)a.dist[o] << 32) | (uint64_t)(p_base + a.pid[o]);
                g = a.group[o];
            }
            const uint64_t T = wave_min_u64(valid && t == b - 1u ? key : ~0ull);
            const bool take = valid && key <= T;
            const uint64_t mt = __ballot(take);
            const uint32_t m = (uint32_t)__popcll(mt);                       // 1 <= m <= 64: the first proposal of an active list is valid
            if (active) cur += (uint32_t)__popcll((mt >> (mine * b)) & (b == 64u ? ~0ull : (1ull << b) - 1ull));
            const uint32_t e = (uint32_t)__popcll(mt & below);
            if (take) {
                tile_key[e] = key;
                tile_grp[e] = g;
            }
            wave_sync();
            uint32_t rank = 0;                                               // (keys of one query are distinct)
            for (uint32_t x = 0; x < m; x++) rank += tile_key[x] < key ? 1u : 0u;
            if (take) {
                sort_key[rank] = key;
                sort_grp[rank] = g;
            }
            wave_sync();
            // lane r: merged position seq + r
            const bool in = lane < m;
            const uint32_t stamp = seq + lane + 1u;                          // <= 64 * 4096
            uint64_t s_key = 0ull;
            uint32_t s_grp = 0u, slot = 0u;
            if (in) {
                s_key = sort_key[lane];
                s_grp = sort_grp[lane];
                slot = grouped_insert(tab, smask, shift, s_grp, stamp);
            }
            wave_sync();
            const bool keep = in && (uint32_t)(tab[slot] >> 32) == stamp;    // the first entry of its group in the merged order
            const uint64_t mk = __ballot(keep);
            const uint32_t pos = kept + (uint32_t)__popcll(mk & below);
            if (keep && pos < k) {
                o_pid[pos] = (uint32_t)s_key;
                o_dist[pos] = (uint32_t)(s_key >> 32);
                o_group[pos] = s_grp;
            }
            kept += (uint32_t)__popcll(mk);
            seq += m;
        }
        const uint32_t total = kept < k ? kept : k;
        for (uint32_t r = total + lane; r < k; r += 64u) {                   // the tail, as idist_search_batch_grouped pads
            o_pid[r] = kInvalid;
            o_dist[r] = 0x7f800000u;
            o_group[r] = 0u;
        }
        if (lane == 0) a.out_count[q] = total;
        if (a.out_counters) {
            c0 = wave_sum_u32(c0); c1 = wave_sum_u32(c1); c2 = wave_sum_u32(c2);
            if (lane < 3) a.out_counters[(size_t)q * 3u + lane] = lane == 0 ? c0 : (lane == 1 ? c1 : c2);
        }
    }
}

}  // namespace idist
