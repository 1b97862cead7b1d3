// idist_mmr.hpp — the kernels of the diverse search (idist_search_batch_mmr, include/idist.h): maximal marginal
// relevance over the candidate list Hnsw::search left on the device.  Of the first m = min(count, fetch) entries of a query's list
// (positions 0..m-1, raw distances d_i) the call selects min(k, m), one per step: position 0 first, then the unselected position with
// the smallest
//
//   score_i = (lambda * d_i) - ((1 - lambda) * m_i),        m_i = min over the selected s of D(i, s),
//
// D the raw canonical distance between the STORED rows of two candidates.  Four f32 operations, each rounded on its own (the library
// is compiled with -ffp-contract=off); scores compare as OrderedFloat does (NaN greatest, all NaNs equal), ties go to the lower
// position: the key  orderable(score) << 32 | position  and an unsigned minimum.
//
// Step t needs only column s_t of D, so a query costs (k - 1) m canonical distances, not m^2 / 2.  The matrix cores do not fit: the
// product form |a|^2 + |b|^2 - 2 a.b rounds differently from the canonical chains, and here the VALUES enter a score — there is no
// verdict that a margin could prove and a canonical pass could confirm, as there is for the reject filter and the build's select
// (DESIGN.md §4.4).  Every D is therefore the chain arithmetic of dist_rounds: the same block order, remaining steps, fold_chains
// and canon_bits, the bits idist_distance_batch returns for the stored row as the query.
//
//   mmr_tile_kernel<NB, RS, TAIL, RPG>   the compile-time geometries.  A workgroup of four waves owns a query; its 32 eight-lane groups
//                           own the pool's rows, group g the positions g, g + 32, ... (RPG of them), each row in dist_rounds' lane
//                           mapping: lane j holds the float4 at t * 32 + j * 4 of every block, its remaining steps and its tail dword.
//                           The pool is read from HBM ONCE, m * 4 * stride bytes per query, every load requested before any is
//                           consumed, and stays in registers for all k steps.  Per step the owner group of the selected position
//                           writes that row to an LDS buffer of `stride` floats (an unrolled, predicated loop over its RPG slots: no
//                           register array is indexed dynamically); after a workgroup barrier every group runs the canonical chain
//                           of each of its rows against the LDS row, block by block — one ds_read_b128 of the LDS row serves the RPG
//                           rows of a lane.  Lane j == 0 of a group keeps d_i, m_i and the selected flags of its rows.  The arg-min is
//                           a u64 minimum inside the wave (wave_min_u64) and across the four waves through four LDS words.
//   mmr_global_kernel<NB, RS, TAIL>      any geometry, any pool up to IDIST_MAX_EF.  One wave per query; ids, d and m live in LDS (a
//                           selected position's id is overwritten with INVALID: that is its flag).  Per step the selected stored
//                           row is staged as the query (it is stored in the blocked order stage_query produces), dist_rounds runs
//                           over the unselected positions from global memory, 64 per batch, and the lanes update m and rank.  It
//                           reads (k - 1) m rows per query from L2 / HBM: the tile kernel's independent ground truth, and the path
//                           of runtime geometries and of pools above the tile's cap.
//
// plan_mmr() chooses between them: a pure host function of the row geometry and the pool size.
//
// POOL = true (idist_partitioned_search_batch_mmr): the candidates' rows live in different parts of a partitioned index, so they were
// gathered into one dense pool first (idist_mmr_pool.hpp) and MmrArgs::r_row names every position's row there.  Both kernels are
// otherwise the same code; with POOL = false nothing of it is compiled in.
#pragma once
#include "idist_grouped_merge.hpp"   // wave_min_u64
#include "idist_search_plan.hpp"

namespace idist {

struct MmrArgs {
    const uint32_t* r_pid;    // [nq][width] the lists of the search
    const uint32_t* r_dist;   // [nq][width] raw distances, f32 bit patterns
    const uint32_t* r_count;  // [nq]
    uint32_t nq, width, k, fetch;
    float lambda, mu;         // mu = 1.0f - lambda, computed once on the host
    uint32_t lam1;            // lambda == 1.0f: the second term is not computed
    uint32_t* o_pid;          // [nq][k]
    uint32_t* o_dist;         // [nq][k] raw d of the selected, f32 bit patterns (the metric's report runs behind the kernel)
    uint32_t* o_rank;         // [nq][k] or nullptr
    uint32_t* o_count;        // [nq]
    const uint32_t* r_row;    // [nq][fetch] POOL kernels: the row of `ix.points` behind every pool position (idist_mmr_pool.hpp); else nullptr
};

// the key of a candidate in the arg-min: OrderedFloat's order of the score as an unsigned order (NaN above +inf, -0 == +0)
__device__ __forceinline__ uint64_t mmr_key(float score, uint32_t pos) {
    uint32_t b = __float_as_uint(score);
    if (b == 0x80000000u) b = 0u;
    uint32_t o = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    if (score != score) o = 0xFFFFFFFFu;
    return ((uint64_t)o << 32) | pos;
}
// (lambda * d) - ((1 - lambda) * m): separate roundings; lambda == 1: lambda * d alone
__device__ __forceinline__ float mmr_score(const MmrArgs& a, float d, float m) {
    const float rel = a.lambda * d;
    if (a.lam1) return rel;
    const float div = a.mu * m;
    return rel - div;
}
// the rows behind a query's selection: INVALID / +inf / INVALID
__device__ __forceinline__ void mmr_pad(const MmrArgs& a, uint32_t q, uint32_t from, uint32_t tid, uint32_t nthreads) {
    for (uint32_t t = from + tid; t < a.k; t += nthreads) {
        a.o_pid[(size_t)q * a.k + t] = kInvalid;
        a.o_dist[(size_t)q * a.k + t] = 0x7f800000u;
        if (a.o_rank) a.o_rank[(size_t)q * a.k + t] = kInvalid;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The tile kernel.  LDS: stride floats (the selected row) + four u64 (the waves' minima).
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr size_t mmr_tile_smem(uint32_t stride) { return (size_t)stride * 4 + 4 * 8; }
#ifdef IDIST_EMU
#define IDIST_MMR_WAVES(W_)
#else
#define IDIST_MMR_WAVES(W_) __attribute__((amdgpu_waves_per_eu(W_, W_)))
#endif

// One step of a canonical chain, acc + (w - p)^2 as dist_rounds computes it: a subtraction and a fused multiply-add.  On the device the
// two instructions are written out: left to itself the compiler pairs the steps of two ROWS into packed f32 instructions, which want
// the two rows' elements in adjacent registers — a second copy of the tile, and with it scratch.  Same operations, same rounding mode.
__device__ __forceinline__ float mmr_chain_step(float w, float p, float acc) {
#ifdef IDIST_EMU
    const float e = w - p;
    return __builtin_fmaf(e, e, acc);
#else
    float e;
    asm("v_sub_f32 %0, %1, %2" : "=v"(e) : "v"(w), "v"(p));
    asm("v_fma_f32 %0, %1, %1, %0" : "+v"(acc) : "v"(e));
    return acc;
#endif
}

template <int NB, int RS, int TAIL, int RPG, int WAVES, bool POOL = false>
__global__ __launch_bounds__(256) IDIST_MMR_WAVES(WAVES) void mmr_tile_kernel(IndexView ix, MmrArgs a) {
    static_assert(NB >= 0 && RS >= 0 && TAIL >= 0 && RPG >= 1 && RPG <= 32, "compile-time layout only");
    IDIST_DYN_SMEM(smem_raw);
    float* row_s = reinterpret_cast<float*>(smem_raw);
    unsigned long long* red = reinterpret_cast<unsigned long long*>(smem_raw + (size_t)ix.stride * 4);
    constexpr int NBA = NB > 0 ? NB : 1, RSA = RS > 0 ? RS : 1;
    const int lane = lane_id();
    const uint32_t wv = threadIdx.x >> 6, gid = wv * 8u + (uint32_t)(lane >> 3);
    const int j = lane & 7;
    for (uint32_t q = blockIdx.x; q < a.nq; q += gridDim.x) {
        block_sync();                                              // the previous query's last reads of row_s / red are done
        uint32_t cnt = a.r_count[q];
        cnt = cnt < a.width ? cnt : a.width;
        const uint32_t m = cnt < a.fetch ? cnt : a.fetch;          // <= 32 * RPG (plan_mmr)
        const uint32_t kk = a.k < m ? a.k : m;
        const uint32_t* l_pid = a.r_pid + (size_t)q * a.width;
        const uint32_t* l_dist = a.r_dist + (size_t)q * a.width;
        // ---- the pool into registers: every load of the tile is requested here, nothing is consumed before the first barrier
        float4 p[RPG][NBA];
        float pr[RPG][RSA], pt[RPG];
        uint32_t pid[RPG];
        float d[RPG], mm[RPG];
        uint32_t live = 0u;                                        // bit r: position gid + 32 r is in the pool and not yet selected
#pragma unroll
        for (int r = 0; r < RPG; r++) {
            const uint32_t i = gid + 32u * (uint32_t)r;
            const bool on = i < m;
            pid[r] = on ? l_pid[i] : kInvalid;
            d[r] = on ? __uint_as_float(l_dist[i]) : 0.0f;
            mm[r] = __uint_as_float(0x7f800000u);
            if (on) live |= 1u << r;
            // one row pointer, immediate offsets, no branch per load.  A slot no group fills (32 r >= m: workgroup-uniform) is
            // skipped; in the last filled slot the groups beyond the pool re-read row 0, never used (n > 0: the row exists; an id
            // outside the index is never dereferenced)
            // (POOL: ix is a view over the row pool of a partitioned index and the row is named by its slot there; the id stays global)
            const uint32_t rw = POOL ? (on ? a.r_row[(size_t)q * a.fetch + i] : kInvalid) : pid[r];
            const float* row = ix.points + (size_t)(on && rw < ix.n ? rw : 0u) * ix.stride + j * 4;
            if (32u * (uint32_t)r < m) {
#pragma unroll
                for (int u = 0; u < NB; u++) p[r][u] = ldg_row4(row + u * 32);
#pragma unroll
                for (int c = 0; c < RS; c++) pr[r][c] = row[NB * 32 + c * 8 - j * 3];
                pt[r] = TAIL ? row[NB * 32 + RS * 8 + (j & 3) - j * 4] : 0.0f;
            } else {
#pragma unroll
                for (int u = 0; u < NB; u++) p[r][u] = float4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int c = 0; c < RS; c++) pr[r][c] = 0.0f;
                pt[r] = 0.0f;
            }
        }
        uint32_t s = 0u;                                           // step 0 selects position 0
        for (uint32_t t = 0; t < kk; t++) {
            // ---- the owner group of s: results out, the flag, and (while a step follows) its row to LDS
            const bool more = t + 1u < kk;
#pragma unroll
            for (int r = 0; r < RPG; r++) {
                if (s == gid + 32u * (uint32_t)r) {
                    live &= ~(1u << r);
                    if (j == 0) {
                        a.o_pid[(size_t)q * a.k + t] = pid[r];
                        a.o_dist[(size_t)q * a.k + t] = __float_as_uint(d[r]);
                        if (a.o_rank) a.o_rank[(size_t)q * a.k + t] = s;
                    }
                    if (more && !a.lam1) {
#pragma unroll
                        for (int u = 0; u < NB; u++) *reinterpret_cast<float4*>(row_s + u * 32 + j * 4) = p[r][u];
#pragma unroll
                        for (int c = 0; c < RS; c++) row_s[NB * 32 + c * 8 + j] = pr[r][c];
                        if (TAIL && j < 4) row_s[NB * 32 + RS * 8 + j] = pt[r];
                    }
                }
            }
            if (!more) break;
            block_sync();
            // ---- D(i, s) of every row of the tile against the LDS row, the chains in dist_rounds' order; m_i
            if (!a.lam1) {
                float acc[RPG];
#pragma unroll
                for (int r = 0; r < RPG; r++) acc[r] = 0.0f;
#pragma unroll
                for (int u = 0; u < NB; u++) {
                    const float4 w = *reinterpret_cast<const float4*>(row_s + u * 32 + j * 4);
#pragma unroll
                    for (int r = 0; r < RPG; r++) {
                        acc[r] = mmr_chain_step(w.x, p[r][u].x, acc[r]);
                        acc[r] = mmr_chain_step(w.y, p[r][u].y, acc[r]);
                        acc[r] = mmr_chain_step(w.z, p[r][u].z, acc[r]);
                        acc[r] = mmr_chain_step(w.w, p[r][u].w, acc[r]);
                    }
                }
#pragma unroll
                for (int c = 0; c < RS; c++) {
                    const float w = row_s[NB * 32 + c * 8 + j];
#pragma unroll
                    for (int r = 0; r < RPG; r++) acc[r] = mmr_chain_step(w, pr[r][c], acc[r]);
                }
                const float qt = TAIL ? row_s[NB * 32 + RS * 8 + (j & 3)] : 0.0f;
#pragma unroll
                for (int r = 0; r < RPG; r++) {
                    const float D = __uint_as_float(canon_bits(fold_chains(acc[r], TAIL != 0, qt, pt[r]), ix.metric));   // valid in lane j == 0
                    mm[r] = D < mm[r] ? D : mm[r];                 // a NaN never lowers it
                }
            }
            // ---- arg-min: the group's best in its lane 0, the wave's, the workgroup's
            uint64_t key = ~0ull;
#pragma unroll
            for (int r = 0; r < RPG; r++) {
                const uint64_t kr = mmr_key(mmr_score(a, d[r], mm[r]), gid + 32u * (uint32_t)r);
                if (j == 0 && ((live >> r) & 1u) && kr < key) key = kr;
            }
            key = wave_min_u64(key);
            if (lane == 0) red[wv] = key;
            block_sync();
            uint64_t best = red[0];
#pragma unroll
            for (int w = 1; w < 4; w++) best = red[w] < best ? red[w] : best;
            s = (uint32_t)best;                                    // (kk <= m: an unselected position exists)
        }
        if (threadIdx.x == 0) a.o_count[q] = kk;
        mmr_pad(a, q, kk, threadIdx.x, 256u);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The global kernel.  LDS: Smem's query row and act lists, then pool ids, d and m (3 * fetch dwords).
// ---------------------------------------------------------------------------------------------------------------------------------
inline size_t mmr_global_smem(uint32_t stride, uint32_t fetch) { return smem_bytes(stride, 0, false, 0, 0, false) + (size_t)fetch * 12; }

template <int NB, int RS, int TAIL, bool POOL = false>
__global__ __launch_bounds__(64) void mmr_global_kernel(IndexView ix, MmrArgs a) {
    IDIST_DYN_SMEM(smem_raw);
    const Smem sm = carve(smem_raw, ix.stride, 0, false, 0, false);
    uint32_t* c_pid = sm.act_dist + 64;
    float* c_d = reinterpret_cast<float*>(c_pid + a.fetch);
    float* c_m = c_d + a.fetch;
    const int lane = lane_id();
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint32_t q = blockIdx.x; q < a.nq; q += gridDim.x) {
        uint32_t cnt = a.r_count[q];
        cnt = cnt < a.width ? cnt : a.width;
        const uint32_t m = cnt < a.fetch ? cnt : a.fetch;
        const uint32_t kk = a.k < m ? a.k : m;
        wave_sync();                                               // the previous query's reads of the pool are done
        for (uint32_t i = (uint32_t)lane; i < m; i += 64u) {
            // (POOL: c_pid holds pool slots — the staged row and dist_rounds' act_pid are slots then; o_pid still comes from r_pid)
            const uint32_t id = POOL ? a.r_row[(size_t)q * a.fetch + i] : a.r_pid[(size_t)q * a.width + i];
            c_pid[i] = id < ix.n ? id : 0u;                        // (an id outside the index is never dereferenced)
            c_d[i] = __uint_as_float(a.r_dist[(size_t)q * a.width + i]);
            c_m[i] = __uint_as_float(0x7f800000u);
        }
        wave_sync();
        uint32_t s = 0u;                                           // step 0 selects position 0
        for (uint32_t t = 0; t < kk; t++) {
            const uint32_t sid = c_pid[s];
            wave_sync();                                           // everybody has read c_pid[s]
            if (lane == 0) {
                a.o_pid[(size_t)q * a.k + t] = a.r_pid[(size_t)q * a.width + s];
                a.o_dist[(size_t)q * a.k + t] = __float_as_uint(c_d[s]);
                if (a.o_rank) a.o_rank[(size_t)q * a.k + t] = s;
                c_pid[s] = kInvalid;                               // selected
            }
            if (t + 1u == kk) break;
            if (!a.lam1) {
                // the stored row is what stage_query makes of the natural one: blocked order, the padding zero
                const float* src = ix.points + (size_t)sid * ix.stride;
                for (uint32_t o = (uint32_t)lane; o < ix.stride; o += 64u) sm.q[o] = src[o];
            }
            wave_sync();
            uint64_t key = ~0ull;
            for (uint32_t base = 0; base < m; base += 64u) {
                const uint32_t i = base + (uint32_t)lane;
                const uint32_t id = i < m ? c_pid[i] : kInvalid;
                const bool un = id != kInvalid;
                float mi = __uint_as_float(0x7f800000u);
                if (!a.lam1) {
                    const uint64_t msk = __ballot(un);
                    const int my = __popcll(msk & below);
                    wave_sync();                                   // the previous batch's act_dist has been read
                    if (un) sm.act_pid[my] = id;
                    wave_sync();
                    dist_rounds<NB, RS, TAIL>(ix, sm.q, sm.act_pid, sm.act_dist, __popcll(msk));
                    wave_sync();
                    if (un) {
                        const float D = __uint_as_float(sm.act_dist[my]);
                        mi = c_m[i];
                        mi = D < mi ? D : mi;                      // a NaN never lowers it
                        c_m[i] = mi;
                    }
                }
                if (un) {
                    const uint64_t kr = mmr_key(mmr_score(a, c_d[i], mi), i);
                    key = kr < key ? kr : key;
                }
            }
            s = (uint32_t)wave_min_u64(key);                       // (kk <= m: an unselected position exists)
        }
        if (lane == 0) a.o_count[q] = kk;
        mmr_pad(a, q, kk, (uint32_t)lane, 64u);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The choice: pure, no HIP call.  The tile serves the compile-time geometries up to 32 * RPG pool positions; RPG is what the register
// budget of `waves` waves per SIMD holds of the geometry's rows (DESIGN.md §4.14 has the compiler's counts).  force: 0 the policy,
// 1 the global kernel, 2 the tile kernel wherever it has an instantiation and the pool fits (`ok` false where it does not).
// ---------------------------------------------------------------------------------------------------------------------------------
// min_fetch: the smallest pool the policy gives the tile.  Its time hardly depends on the pool (every slot of the tile is computed, a
// workgroup per query), the global kernel's grows with it.  Each is the smallest MEASURED pool at which every reading of the tile was
// below every reading of the global kernel (fetch 32 / 64 / 100, 10k queries, k 10, the kernels alternately: profiles/mmr_search.json,
// DESIGN.md §4.14): 128-d slower at 32 and 64, ahead at 100; 300-d level at 32, ahead at 64 and 100; 768-d slower at 32, ahead at 64
// and 100.  Between two measured pools nothing is claimed, so the global kernel keeps them.
template <int NB> struct MmrTile { static constexpr int rpg = 0, waves = 1, min_fetch = 0; };                // runtime geometries: no tile
template <> struct MmrTile<4> { static constexpr int rpg = 8, waves = 2, min_fetch = 100; };                 // 128-d: 8 x 16 data registers
template <> struct MmrTile<9> { static constexpr int rpg = 4, waves = 2, min_fetch = 64; };                  // 300-d: 4 x 38
template <> struct MmrTile<24> { static constexpr int rpg = 4, waves = 1, min_fetch = 64; };                 // 768-d: 4 x 96, one 512-register wave per SIMD
struct MmrPlan {
    bool tile = false, ok = true;
    uint32_t rpg = 0, waves = 0;     // tile: rows per group, waves per SIMD (= resident workgroups per CU)
    uint32_t min_fetch = 0;
};
inline MmrPlan plan_mmr(const Layout& L, uint32_t fetch, int force = 0) {
    MmrPlan p;
#define IDIST_MMR_GEO(L_, CALL_, NB_, RS_, TAIL_) \
    if ((L_).nb == (NB_) && (L_).rs == (RS_) && (L_).tail == (TAIL_)) { p.rpg = MmrTile<NB_>::rpg; p.waves = MmrTile<NB_>::waves; p.min_fetch = MmrTile<NB_>::min_fetch; }
    IDIST_GEO_LIST(IDIST_MMR_GEO, L, _)
#undef IDIST_MMR_GEO
    const bool can = p.rpg != 0 && fetch <= 32u * p.rpg;
    p.tile = can && (force == 2 || (force == 0 && fetch >= p.min_fetch));
    p.ok = force != 2 || can;
    return p;
}

}  // namespace idist
