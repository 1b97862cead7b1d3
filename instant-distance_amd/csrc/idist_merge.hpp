// idist_merge.hpp — the union step of a partitioned index: P sorted result lists per query -> the best out_width of all.
//
// A partitioned search runs Hnsw::search on every part; each part returns <= width (PointId, distance) pairs, nearest first.
// The answer is the merge of those lists by the reference's `Candidate` order (core/types.rs:229-234: distance, then id) with
// ids translated to global ids (base[p] + pid).  Distances arrive canonical (canon_bits: non-negative, every NaN = kNanBits),
// so the unsigned order of the 64-bit key  dist_bits << 32 | global id  IS that order, and all keys of a query are distinct.
//
// Every list is sorted, so an element's place in the merged order is known without merging anything:
//     rank = (its index in its own list) + sum over the other lists of (number of keys below it),
// each term one binary search.  An element with rank < out_width stores itself at out[rank]: no atomics, no ordering between
// lanes, the same bytes whatever the schedule.  Only the first min(count, width, out_width) entries of a list can matter — an
// element at index >= out_width ranks >= out_width, and a list that holds out_width keys below an element pushes it out by
// itself — so lists are cut there.  The lists' COUNTS rule, never their padding (a +inf pad would sort before a real NaN).
//
// One wave per query.  The query's P * width keys are staged once into LDS as u64 (16-byte loads of the pid and distance rows
// when width is a multiple of four) and the binary searches run against LDS; when they do not fit the workgroup's LDS budget the
// same code reads the lists where they are (they were just written: L2-resident) — correct up to 64 x 4096 keys, not fast.
// The probes of a binary search are data dependent: its first steps read one address per list (a broadcast), the last ones
// scatter over the banks; no layout of sorted keys avoids that, and the kernel is a few per cent of the walks it follows.
#pragma once
#include "idist_device.hpp"

namespace idist {

constexpr uint32_t kMergeMaxLists = 64;           // one lane per list holds its count, base and counters
constexpr uint32_t kMergeHeadBytes = 512;         // LDS: len[64], base[64] (u32) in front of the keys
constexpr uint32_t kMergeLdsBudget = 64 * 1024;   // per workgroup (= per query in flight); P = 8, ef = 100 uses 6.9 KB

struct MergeArgs {
    const uint32_t* pid;        // [n_lists][nq][width]
    const uint32_t* dist;       // [n_lists][nq][width] f32 bit patterns
    const uint32_t* count;      // [n_lists][nq]
    const uint32_t* counters;   // [n_lists][nq][3] or nullptr
    uint32_t n_lists, nq, width, out_width;
    uint32_t* out_pid;          // [nq][out_width]
    uint32_t* out_dist;         // [nq][out_width] f32 bit patterns
    uint32_t* out_count;        // [nq]
    uint32_t* out_counters;     // [nq][3] or nullptr
    uint32_t vec4;              // width % 4 == 0 and both input rows 16-byte aligned: stage with 16-byte loads
    uint32_t base[kMergeMaxLists];
};

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}

template <bool LDS>
__global__ __launch_bounds__(64) void merge_topk_kernel(MergeArgs a) {
    IDIST_DYN_SMEM(smem_raw);
    uint32_t* len_s = reinterpret_cast<uint32_t*>(smem_raw);
    uint32_t* base_s = len_s + kMergeMaxLists;
    uint64_t* keys_s = reinterpret_cast<uint64_t*>(smem_raw + kMergeHeadBytes);
    const int lane = lane_id();
    const uint32_t P = a.n_lists, w = a.width, wo = a.out_width, nq = a.nq;
    const uint32_t wl = w < wo ? w : wo;          // no list matters beyond this index
    base_s[lane] = (uint32_t)lane < P ? a.base[lane] : 0u;
    for (uint32_t q = blockIdx.x; q < nq; q += gridDim.x) {
        wave_sync();                              // the previous query's searches are done with len_s / keys_s
        uint32_t c = 0, c0 = 0, c1 = 0, c2 = 0;
        if ((uint32_t)lane < P) {
            c = a.count[(size_t)lane * nq + q];
            c = c < w ? c : w;
            if (a.counters) {
                const uint32_t* s = a.counters + ((size_t)lane * nq + q) * 3u;
                c0 = s[0]; c1 = s[1]; c2 = s[2];
            }
        }
        len_s[lane] = c < wl ? c : wl;
        const uint32_t total = wave_sum_u32(c);   // <= 64 * 4096
        if (a.out_counters) {
            c0 = wave_sum_u32(c0); c1 = wave_sum_u32(c1); c2 = wave_sum_u32(c2);
            if (lane < 3) a.out_counters[(size_t)q * 3u + lane] = lane == 0 ? c0 : (lane == 1 ? c1 : c2);
        }
        if (LDS) {
            if (a.vec4) {
                for (uint32_t e = 4u * lane; e < P * w; e += 256u) {
                    const uint32_t p = e / w, i = e - p * w;
                    const size_t o = ((size_t)p * nq + q) * w + i;
                    const uint4 id = *reinterpret_cast<const uint4*>(a.pid + o);
                    const uint4 d = *reinterpret_cast<const uint4*>(a.dist + o);
                    const uint32_t b = base_s[p];
                    keys_s[e + 0] = ((uint64_t)d.x << 32) | (uint64_t)(b + id.x);
                    keys_s[e + 1] = ((uint64_t)d.y << 32) | (uint64_t)(b + id.y);
                    keys_s[e + 2] = ((uint64_t)d.z << 32) | (uint64_t)(b + id.z);
                    keys_s[e + 3] = ((uint64_t)d.w << 32) | (uint64_t)(b + id.w);
                }
            } else {
                for (uint32_t e = lane; e < P * w; e += 64u) {
                    const uint32_t p = e / w, i = e - p * w;
                    const size_t o = ((size_t)p * nq + q) * w + i;
                    keys_s[e] = ((uint64_t)a.dist[o] << 32) | (uint64_t)(base_s[p] + a.pid[o]);
                }
            }
        }
        wave_sync();
        auto key_at = [&](uint32_t p, uint32_t i) -> uint64_t {
            if (LDS) return keys_s[p * w + i];
            const size_t o = ((size_t)p * nq + q) * w + i;
            return ((uint64_t)a.dist[o] << 32) | (uint64_t)(base_s[p] + a.pid[o]);
        };
        uint32_t* o_pid = a.out_pid + (size_t)q * wo;
        uint32_t* o_dist = a.out_dist + (size_t)q * wo;
        for (uint32_t e = lane; e < P * wl; e += 64u) {
            const uint32_t p = e / wl, i = e - p * wl;
            if (i >= len_s[p]) continue;
            const uint64_t key = key_at(p, i);
            uint32_t rank = i;
            for (uint32_t p2 = 0; p2 < P && rank < wo; p2++) {
                if (p2 == p) continue;
                uint32_t lo = 0, hi = len_s[p2];  // number of keys of list p2 below mine (keys are distinct)
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (key_at(p2, mid) < key) lo = mid + 1u;
                    else hi = mid;
                }
                rank += lo;
            }
            if (rank < wo) {
                o_pid[rank] = (uint32_t)key;
                o_dist[rank] = (uint32_t)(key >> 32);
            }
        }
        const uint32_t outc = total < wo ? total : wo;
        for (uint32_t r = outc + lane; r < wo; r += 64u) {   // the tail, as idist_search_batch pads
            o_pid[r] = kInvalid;
            o_dist[r] = 0x7f800000u;
        }
        if (lane == 0) a.out_count[q] = outc;
    }
}

}  // namespace idist
