// idist_search_plan.hpp — which search_kernel answers a batch, with which visited set, LDS and residency: the decision alone.
// plan_search() is a pure function of plain values (SearchFacts, Knobs): no HIP call, no index, no context, no allocation, no error
// path.  launch_search (idist_capi.hip) gathers the facts, makes the tables the plan wants and launches what it names;
// tests/host/search_plan.cpp compiles this header alone and holds the policy against a recorded table (tests/golden/search_plan.txt).
#pragma once
#include "idist_kernels.hpp"

#include <algorithm>

namespace idist {

struct Layout {
    uint32_t stride, nb, rs, tail;
};
inline Layout make_layout(uint32_t dim) {
    const uint32_t dp = (dim + 3u) & ~3u;      // zero padding is a bitwise no-op (fma(0,0,acc) == acc)
    const uint32_t steps = dp / 8u;            // chunks_exact(8), instant-distance-py/src/lib.rs:391
    Layout L;
    L.tail = (dp % 8u) == 4u ? 1u : 0u;        // :402-405
    L.nb = steps / 4u;
    L.rs = steps % 4u;
    const uint32_t used = 32u * L.nb + 8u * L.rs + 4u * L.tail;
    L.stride = std::max(16u, (used + 15u) & ~15u);
    return L;
}

// The row geometries the kernels are instantiated for at compile time — ONE list: IDIST_DISPATCH instantiates them, and every
// policy that asks "is this a runtime-geometry index?" (plan_search, run_build, filter_applies) asks has_template_geometry().
#define IDIST_GEO_LIST(X, L, CALL) X(L, CALL, 4, 0, 0) /* dim 128 */ X(L, CALL, 9, 1, 1) /* dim 300 */ X(L, CALL, 24, 0, 0) /* dim 768 */
#define IDIST_GEO_TEST(L, CALL, NB_, RS_, TAIL_) if ((L).nb == (NB_) && (L).rs == (RS_) && (L).tail == (TAIL_)) return true;
inline bool has_template_geometry(const Layout& L) {
    IDIST_GEO_LIST(IDIST_GEO_TEST, L, _)
    return false;
}
#define IDIST_GEO_CASE(L, CALL, NB_, RS_, TAIL_) \
    if (!idist_geo_hit_ && (L).nb == (NB_) && (L).rs == (RS_) && (L).tail == (TAIL_)) { idist_geo_hit_ = true; CALL(NB_, RS_, TAIL_); }
#define IDIST_DISPATCH(L, CALL)                                         \
    do {                                                                \
        bool idist_geo_hit_ = false;                                    \
        IDIST_GEO_LIST(IDIST_GEO_CASE, L, CALL)                         \
        if (!idist_geo_hit_) { CALL(-1, -1, -1); }                      \
    } while (0)

// Which filtered kernels a row geometry can ever be given (plan_search / run_build): instantiating only those keeps the build of
// the library's translation unit at three minutes.  The thin filtered walk serves compact rows of up to five chunks (128-d, 300-d, runtime
// geometries) — on the identity rows, and a second instantiation on the 64-byte principal rows (walk_thin_filter_principal) — one fat
// filtered wave per SIMD the longer ones (768-d, runtime geometries); descents are filtered on thin waves only.  A launch the policy asks for and the geometry has no kernel for is an internal error, never a silent no-op.
template <int NB> struct GeoKernels {
    static constexpr bool thin_search = NB != 24;
    static constexpr bool fat_filtered_search = NB == 24 || NB < 0;
    static constexpr bool fat_filtered_search_ids = NB == 24;      // (the id form of the set, cheaper to probe while a walk cannot fill it: C4)
    // thin filtered descents: rows of at least 192 floats by policy — 128-d rows only under the test knob IDIST_BUILD_FILTER=1
#if defined(IDIST_VARIANTS) || defined(IDIST_EMU) || defined(IDIST_PROBE)
    static constexpr bool thin_descent = true;
#else
    static constexpr bool thin_descent = NB != 4;
#endif
};
// the reject filter has a kernel for this index: a template geometry, or compact rows within the fat filtered wave's tile
inline bool filter_applies(uint32_t n, const Layout& L) {
    return n > 0 && (has_template_geometry(L) || filt_stride(L.stride) <= 128u * (uint32_t)kFiltRtChunksFat);
}

// Knobs read from the environment (knobs_from_env, idist_capi.hip: three in the product, the rest in the test / measurement builds),
// sampled once per context or build — not per launch.
struct Knobs {
    uint32_t latency_nq = 1024;   // IDIST_LATENCY_NQ: batches up to this many queries run the latency walk (0 = never)
    bool classic = false;         // IDIST_WALK=classic
    bool bloom = true;            // IDIST_BLOOM=0 disables the LDS Bloom filter in front of the visited bitmap
    uint32_t tab_log2 = 0;        // IDIST_TAB_LOG2=<5..13>: size of the on-chip visited set (test knob: small sets exercise the overflow path)
    bool vis_bitmap = false;      // IDIST_VISITED=bitmap: search with bitmap + Bloom filter (16 waves per CU) instead of the on-chip set
    bool vis_onchip = false;      // IDIST_VISITED=onchip: the on-chip set whatever the policy says (test / A-B knob)
    bool combine = true;          // IDIST_COMBINE=0: every scalar host-pointer call makes its own launch, however many are in flight
    bool sync_flag = true;        // IDIST_SYNC=stream: narrow host-pointer calls wait with hipStreamSynchronize instead of for the completion
                                  // word the kernel writes to the context's pinned buffer (A/B knob)
    bool tie_spill_first = false; // IDIST_TIE_SPILL=1: strict ties go to the HBM bags at the first overflow instead of growing the LDS region first (test knob)
    bool events = true;           // IDIST_KERNEL_EVENTS=0: no HIP events around the search kernels (idist_search_ctx_kernel_times then has nothing)
    bool filter = true;           // IDIST_FILTER=0: wide on-chip walks without the reject filter (test / A-B knob)
    uint32_t filter_waves = 0;    // IDIST_FILTER_WAVES=2|3: thin waves per SIMD of a walk on the principal rows (A/B knob; 0: kFilterWavesPrincipal)
    int basis = 0;                // IDIST_FILTER_BASIS=identity|principal: the compact rows thin wide searches read, whatever the index's
                                  // policy chose (principal: where the index is eligible for that table) (test / A-B knob)
    int inl = -1;                 // IDIST_FILTER_INLINE=0|1: thin principal walks without / with the principal rows stored with the adjacency
                                  // (A/B knob; -1: kFilterInlinePolicy)
    bool tab_ids = false;         // IDIST_TAB_FORMAT=ids: the on-chip set always keeps full ids (4 per bucket, frozen at 7/8), never
                                  // 16-bit quotients (8 per bucket, single ids overflow) (test / A-B knob)
    bool tab_q16 = false;         // IDIST_TAB_FORMAT=q16: quotients wherever they apply, also where the policy would keep ids
    bool no_zero_copy = false;    // IDIST_NO_ZERO_COPY=1: narrow host-pointer batches take the general (staged) path too (test / A-B knob)
    int ea = 0;                   // IDIST_EA=<k> (measurement builds only, -DIDIST_EA_PROBE): early abandon after k blocks of a 300-d row
    uint32_t w2_ef = 0xFFFFFFFFu; // IDIST_W2_EF=<ef>: from this ef_search on, wide on-chip batches run two 256-register waves per SIMD (A/B knob; default: policy)
    uint32_t allowed_segments = 0;    // IDIST_ALLOWED_SEGMENTS=<1..64>: segments of the exact step of a restricted search (test knob: the result
                                      // must not depend on it; default: by the number of pending queries)
    uint32_t range_segments = 0;      // IDIST_RANGE_SEGMENTS=<1..64>: segments of the exact step of a range search (test knob, as allowed_segments)
    uint64_t grouped_stage = 0;       // IDIST_GROUPED_STAGE=<bytes>: staging bound of the bitmaps of an exact round of a grouped search (test
                                      // knob: small bounds cut the pending queries into chunks; the result must not depend on it; default 256 MiB)
    uint32_t range_sort_chunk = 0;    // IDIST_RANGE_SORT_CHUNK=<128..4096, a power of two>: keys a wave of the range search's sort holds in
                                      // LDS (test knob: small chunks send short lists through the global-memory strides; default 2048)
    uint32_t quad_nq = 0xFFFFFFFFu;   // IDIST_QUAD_NQ: batches up to this many queries run four waves per query (default: two
                                      // workgroups per CU, one for 768-d rows; 0 = never)
    // the build's (plan_build, idist_build_plan.hpp; all test / A-B knobs: every variant builds the same graph)
    uint32_t build_rt = 8;            // IDIST_BUILD_RT=<rows>: rows of the update tile (step B2) before the LDS budget trims them
    uint32_t build_rt2 = 16;          // IDIST_BUILD_RT2=<rows>: ... of the select tile (step A2)
    bool build_a2_tile = false;       // IDIST_BUILD_A2=tile: step A2 with the LDS-tile kernel, never the Gram matrix on MFMA
    bool build_pipeline = true;       // IDIST_BUILD_PIPELINE=0: the sequential schedule
    uint32_t build_a_waves = 0;       // IDIST_BUILD_A_WAVES=<1..8>: descent waves per CU of a pipelined step (0: policy)
    int build_a_regs = -1;            // IDIST_BUILD_A_REGS=256|512: the descents' register budget (-1: policy)
    bool build_quad = true;           // IDIST_BUILD_QUAD=0: narrow steps never run four waves per insertion
    uint32_t build_growth = 8;        // IDIST_BUILD_GROWTH=<8..32>: narrow steps hold g / this many insertions
    int build_streams = 1;            // IDIST_BUILD_STREAMS=off (0) | narrow (1) | all (2): which steps take the extra streams
    int build_filter = -1;            // IDIST_BUILD_FILTER=0|1: descents never / wherever it applies with the reject filter (-1: policy)
    bool build_dlog = true;           // IDIST_BUILD_NO_DLOG: the descents log no distances for step B
    uint32_t build_chunk = 0;         // IDIST_BUILD_CHUNK=<items>: step B's items per dequeue (0: by load)
    bool build_no_fast = false;       // IDIST_BUILD_NO_FAST: every update through B2
    bool build_check = false;         // IDIST_BUILD_CHECK: a pipelined build ends by comparing the two copies of the zero layer
};

// the compact rows' formats as an index records them (SearchFacts::filt_format, Knobs::basis); include/idist.h's IDIST_FILTER_FORMAT_*
// (idist_capi.hip asserts that they agree)
enum : int { kFilterFormatNone = 0, kFilterFormatIdentity = 1, kFilterFormatPrincipal = 2 };

// Everything the policy reads: of the index, of the call and its context, and of the lazily made tables as they stand.
struct SearchFacts {
    uint32_t n = 0;
    Layout L{};
    int n_cu = 256;
    bool template_geometry = false;   // has_template_geometry(L)
    bool filter_applies = false;      // filter_applies(n, L)
    uint32_t ef = 0, nq = 0;
    uint32_t tie_cap = 0;             // max(the config's tie capacity, what the context has grown to)
    uint32_t dirty_words = 0;         // VisGeom::dirty_words of the context
    bool filter_ready = false;        // the identity table stands (filt_state == 1)
    bool principal_table = false;     // ... and the principal table beside it
    int filt_format = kFilterFormatNone;   // the format the index's policy chose for thin wide searches
    bool inline_ready = false;        // the principal rows stored with the adjacency stand (filt_inl_state == 1)
};

// one value per kernel choice of launch_search's switch, in the order the rules below test them
enum class SearchWalk : int {
    QuadQ16, QuadIds,                                                     // four waves per query (narrow batches)
    ThinPrincipal3, ThinInline, ThinPrincipal, ThinIdentity,              // thin filtered waves
    ClassicOnChipQ16,                                                     // (test builds)
    TwoPerSimd,
    FatFilteredIds, FatFilteredQ16,
    OnChipQ16,
    ClassicOnChipIds,                                                     // (test builds)
    OnChipIds,
    Latency,
    ClassicBitmap,                                                        // (test builds)
    OverlapBitmap,
    kCount
};
inline const char* walk_name(SearchWalk w) {
    static const char* const names[] = {"quad_q16", "quad_ids", "thin_principal3", "thin_inline", "thin_principal", "thin_identity",
                                        "classic_on_chip_q16", "two_per_simd", "fat_filtered_ids", "fat_filtered_q16", "on_chip_q16",
                                        "classic_on_chip_ids", "on_chip_ids", "latency", "classic_bitmap", "overlap_bitmap"};
    static_assert(sizeof(names) / sizeof(names[0]) == (size_t)SearchWalk::kCount, "one name per walk");
    return names[(int)w];
}
constexpr bool plan_thin(SearchWalk w) { return w >= SearchWalk::ThinPrincipal3 && w <= SearchWalk::ThinIdentity; }
constexpr bool plan_fat_filtered(SearchWalk w) { return w == SearchWalk::FatFilteredIds || w == SearchWalk::FatFilteredQ16; }
// the walk keeps 16-bit quotients in its on-chip set
constexpr bool plan_q16(SearchWalk w) {
    return w == SearchWalk::QuadQ16 || plan_thin(w) || w == SearchWalk::ClassicOnChipQ16 || w == SearchWalk::TwoPerSimd ||
           w == SearchWalk::FatFilteredQ16 || w == SearchWalk::OnChipQ16;
}

// the FilterViews the launch's IndexView carries
enum class PlanFilter : int { None, Identity, Principal };   // Principal: IndexView::f the principal rows, f2 the identity rows

struct SearchPlan {
    SearchWalk walk = SearchWalk::OverlapBitmap;
    uint32_t block = 64;              // threads per workgroup: 256 for the four-wave walks
    uint32_t tab_log2 = 0, ubits = 0; // SearchArgs: the on-chip set (0: none) and the universe of its quotients
    uint32_t wcap = 0;
    uint32_t resident = 0;            // workgroups the chip holds at once (before the tie bags' clamp)
    size_t smem = 0;
    PlanFilter filter = PlanFilter::None;
    bool inl = false;                 // IndexView::inl
    bool wants_filter = false;        // the walk is a filtered one where the index has the table: make it first (filter_ensure)
    bool wants_inline = false;        // ... and the inlined blocks (filter_inline_ensure)
    bool lds_short = false;           // smem > 64 KiB: this ef_search does not fit a wave's LDS, nothing can be launched
};

// LDS one wave of the on-chip walk may use: one wave per SIMD, four per CU, out of 160 KiB
constexpr size_t kOnChipLdsPerWave = 40 * 1024;

// Which walk serves a wide batch (profiles/r02/probe_r02_ef_paths_onchip_vs_bitmap.jsonl, probe_r02_configs_c2_c4_c5.jsonl):
//   * a search visits ~53 * ef_search + 600 nodes; the 8192-id on-chip set is frozen at 7168 and the rest of the walk
//     test-and-sets the bitmap.  The fat on-chip waves still win while a row fetch outweighs that extra round trip:
//     up to ef_search ~ 180 at 128-d, ~ 550 at 300-d (id set; ~ 600 with the quotient set), beyond 200 at 768-d;
//   * an index that sits in the Infinity Cache (100k x 128: 51 MB) is served faster by 16 small waves per CU
//     (4.2 vs 5.0 ms per 10k queries): the on-chip walk is for HBM-resident indexes.
//   * round 4 (profiles/r04/probe_r04f_ef_crossover_c3.jsonl, probe_r04i_ef_paths_wide_merge_c3.jsonl): with the quotient set the
//     crossover at 300-d moved from ~1.5 to ~2 x row floats, and once the fat waves merged a `nearest` of up to 1024 entries in
//     one pass (w_push_merge<16>) the on-chip walk stayed ahead of the bitmap walk up to ef_search 1000 (0.651 / 0.637 / 0.625
//     vs 0.628 / 0.620 / 0.611 of spec at 650 / 800 / 1000; beyond the merge's reach too: 0.628 vs 0.565 at ef 1000 in
//     probe_r04k).  Rows of >= 256 floats: on chip as far as LDS allows; shorter rows: the line through the 128-d (~180) and
//     300-d (~600) crossovers.
//   * round 5 (profiles/r05/probe_r05m_walk_policy_cache_resident.jsonl, probe_r05n_walk_policy_by_size_and_row.jsonl: on-chip walk vs
//     bitmap walk at 9 more shapes): which walk wins near the Infinity Cache depends on the ROW LENGTH, not on residency alone.
//     Rows of >= 256 floats: the on-chip walk wins by 5-8 % also where the index sits in the cache (100k x 300: 7.97 vs 8.51 ms,
//     40k x 768: 17.2 vs 18.1 ms per 10k queries at ef 100; the same at ef 150-800).  Shorter rows: the bitmap walk wins well BEYOND
//     the 128-MB mark — 300k x 128 (154 MB): 4.39 vs 4.69 ms at ef 100, 6.03 vs 7.50 at ef 150; 400k x 200-d (320 MB): 7.49 vs 8.76 and
//     13.2 vs 17.8; 1M x 64-d (256 MB): 4.96 vs 6.84 — and loses from ~512 MB on (1M x 128: 6.73 vs 5.29 ms); and once such an index
//     is far beyond the cache the on-chip walk stays ahead to higher ef_search (1M / 2M x 128 at ef 200: 10.6 / 10.9 against 11.8 /
//     15.0 ms; 2M x 128 at ef 400: 23.0 against 27.5; 1M x 128 at ef 400: a tie).
//     Runtime-geometry rows shorter than 128 floats are different again: the fat waves' register tile (<8 blocks, 4 rounds>) keeps only
//     4 x 8 rows x 256 B = 8 KB on the wire per wave at 64-d, and the bitmap walk wins at EVERY size — 4M x 64 (1 GB): 5.93 / 10.7 /
//     20.1 ms against 7.13 / 14.9 / 31.0 ms at ef 100 / 200 / 400; at 100-d (3 blocks) it wins from ef ~150 on (3M x 100: 14.9 / 27.3
//     against 16.3 / 34.0 ms at ef 200 / 400, a tie at ef 100); 200-d rows behave like the 128-d instantiation (2M x 200: on chip 9.83 /
//     19.3 against 11.5 / 21.1 ms) — profiles/r05/probe_r05u_walk_policy_short_rt_rows_large.jsonl.
inline uint32_t on_chip_max_ef(uint32_t stride_floats, size_t index_bytes, bool runtime_geometry) {
    if (stride_floats >= 256u) return 1536u;       // (as far as W and the set fit a wave's LDS: tab_fit in plan_search)
    if (runtime_geometry && stride_floats <= 64u) return 0u;         // never: see above
    if (runtime_geometry && stride_floats < 128u) return 160u;
    const int ef = (int)stride_floats * 61 / 25 - 132;
    return (uint32_t)std::min(1536, std::max(index_bytes >= ((size_t)512 << 20) ? 400 : 160, ef));
}
// short rows (< 256 floats) are served by the bitmap walk up to this many bytes of point rows (see above)
constexpr size_t kShortRowBitmapBytes = (size_t)320 << 20;
// ... and long rows by the on-chip walk from this size on (below it nothing was measured: the round-2 rule stands)
constexpr size_t kLongRowOnChipBytes = (size_t)96 << 20;
constexpr uint32_t kFilterWaves = 2u;    // waves per SIMD of a filtered wide walk (plan_search)
constexpr uint32_t kFilterWavesPrincipal = 2u;   // ... on the principal rows (three: measured)
constexpr bool kFilterInlinePolicy = true;       // thin principal walks read the blocks stored with the adjacency where the index has them
constexpr uint32_t kLongWalkEf = 512u;   // ef_search from which wide on-chip batches run two thinner waves per SIMD (see plan_search)

inline SearchPlan plan_search(const SearchFacts& f, const Knobs& knobs) {
    SearchPlan p;
    const uint32_t ef = f.ef, nq = f.nq;
    const Layout& L = f.L;
    p.wcap = ef + 64 + f.tie_cap + 8;
    // this launch's LDS with a visited set (or Bloom filter) of 2^l words, with or without the four-wave walk's hand-over block
    const auto lds = [&](uint32_t l, bool hand_over = true) { return smem_bytes(L.stride, p.wcap, false, 1u << l, f.dirty_words, hand_over); };
    // Default walk: the visited set lives in LDS (an exact hash set of 2^tab_log2 ids per query, the HBM bitmap only
    // takes what does not fit), one wave per SIMD with up to 512 registers for rows in flight.  The largest set that
    // fits a quarter of the CU's LDS next to the query tile and W is used; none fits (huge ef_search) -> bitmap walk.
    uint32_t tab_fit = 0;                                               // largest set that fits at all
    for (uint32_t l = 13; l >= 10 && !tab_fit; l--)
        if (lds(l) <= kOnChipLdsPerWave) tab_fit = l;
    if (tab_fit && knobs.tab_log2) tab_fit = std::min(tab_fit, knobs.tab_log2);
    if (knobs.vis_bitmap) tab_fit = 0;
    // Narrow batches (the reference's call pattern is ONE query per Hnsw::search): a four-wave workgroup per query,
    // one workgroup per CU — the rows of an expansion are fetched by all four SIMDs in one round trip.
    // Two such workgroups share a CU where the kernel's registers allow it (all but the 768-d instantiation): up to two
    // queries per CU the four-wave walk beats the single-wave one (512 queries: 0.65 vs 0.81 ms at C3), beyond it loses.
    const uint32_t quad_per_cu = (L.nb == 24 && L.rs == 0 && L.tail == 0) ? 1u : 2u;
    const uint32_t quad_nq = knobs.quad_nq == 0xFFFFFFFFu ? (uint32_t)f.n_cu * quad_per_cu : knobs.quad_nq;
    const bool quad = tab_fit && !knobs.classic && nq <= quad_nq;
    const size_t row_bytes = (size_t)f.n * L.stride * 4;
    const bool long_rows = L.stride >= 256u;
    const bool rt_rows = !f.template_geometry;   // no compile-time instantiation of the row geometry
    const bool cache_resident = long_rows ? row_bytes < kLongRowOnChipBytes : row_bytes <= kShortRowBitmapBytes;   // "served best by many small waves"
    // With the reject filter in front (round 6) the on-chip walk stays ahead at every ef_search the set fits — 1M x 128 at ef 200 / 400:
    // 8.5 / 15.4 ms against 10.6 / 20.8 ms on the bitmap walk, 4M x 64-d at ef 100 / 200: 5.1 / 10.3 against 5.9 / 11.8 — and the ef
    // caps of on_chip_max_ef only bind for unfiltered indexes (compact rows beyond the filter's tiles, IDIST_FILTER=0).  The
    // cache-residency rule shrinks too: filtered long rows take it at every size (20k x 300: 3.46 against 5.87 ms; 40k x 768 did before),
    // filtered short rows from the L2's reach on (8 x 4 MB: 100k x 128 = C2 3.44 against 3.80 ms at ef 100, 6.56 against 6.64 at ef 200,
    // a tie at 400; 300k x 128 3.65 against 4.45; 400k x 200-d 4.71 against 7.48) — below it the bitmap walk's sixteen small waves per
    // CU win (10k x 128: 1.98 against 2.83 ms, 50k x 64-d: 2.85 against 3.75) — profiles/probe_r06f_filter_policy.jsonl,
    // probe_r06l_c2_policy.jsonl.
    const bool filter_ok = knobs.filter && f.filter_applies;
    const bool small_for_filter = !long_rows && row_bytes < ((size_t)32 << 20);
    const bool wide_on_chip = tab_fit && (knobs.vis_onchip || knobs.tab_log2 ||
                                          (filter_ok ? !small_for_filter : (ef <= on_chip_max_ef(L.stride, row_bytes, rt_rows) && !cache_resident)));
    const bool on_chip = quad || wide_on_chip;
    uint32_t tab_log2 = on_chip ? tab_fit : 0u;
    // The reject filter in front of the wide on-chip walks' distance passes (its compact rows are made on first use).  A filtered
    // walk is bound by its dependent round trips, so it runs as `fw` thin waves per SIMD (walk_thin_filter, idist_device.hpp) with
    // the largest quotient set that lets 4 * fw of them share a CU's LDS — where the quotient form applies (n <= 33M) and the
    // caller did not pin the set's form or size.
    const bool use_filter = wide_on_chip && !quad && filter_ok;
    p.wants_filter = use_filter;
    const bool filtered = use_filter && f.filter_ready;
    // (every other wide walk — unfiltered indexes, IDIST_TAB_FORMAT=ids, the classic test walks, n beyond the quotient form's reach —
    //  runs the round-5 kernels, compiled WITHOUT the filter: carrying its registers cost the 1024-d search 15 %)
    // Long rows (compact rows beyond the thin tile's five chunks: 768-d) keep ONE fat wave per SIMD with the filter: a thin wave's registers hold 16
    // of their compact rows and a quarter of an f32 row at a time — six or seven dependent round trips per expansion where the fat
    // wave makes two (C5, ef 200: 162 ms fat against 213 ms thin per 65,536 queries; C4 a tie at 78-83 ms).
    // (always on the quotient form of the set — the id form's cheaper probe was worth 1-2 % and another two large kernels to compile)
    const bool fat_filtered = filtered && !knobs.classic && !knobs.tab_ids && filt_stride(L.stride) > 128u * (uint32_t)kFiltRtChunks &&
                              q16_applies(tab_fit, q16_universe_bits(f.n, tab_fit));
    // ... except the 768-d instantiation while the id form of the set cannot fill up (ef_search <= ~120: C4)
    const bool fat_ids = fat_filtered && L.nb == 24 && L.rs == 0 && L.tail == 0;
    uint32_t fw = 1;
    // thin walks read the table the index's policy chose (filter_principal_ensure) — the 64-byte principal rows have their own instantiation
    const bool principal_rows = filtered && !fat_filtered && f.principal_table &&
                                (knobs.basis ? knobs.basis : f.filt_format) == kFilterFormatPrincipal;
    if (filtered && !fat_filtered && !knobs.classic && !knobs.tab_ids)
        fw = principal_rows ? (knobs.filter_waves ? knobs.filter_waves : kFilterWavesPrincipal) : kFilterWaves;
    if (fw > 1) {
        uint32_t l = knobs.tab_log2 ? std::min(tab_fit, knobs.tab_log2) : tab_fit;
        // (a smaller set addresses fewer ids in its 16-bit quotients: 10M points need the 16-KB set — C5 runs six or seven thin
        //  waves per CU on it rather than eight on a set it cannot use)
        while (l > 10u && lds(l, false) * 4u * fw > (size_t)160 * 1024 && q16_applies(l - 1u, q16_universe_bits(f.n, l - 1u)))
            l--;
        if (q16_applies(l, q16_universe_bits(f.n, l))) tab_log2 = l;
        else fw = 1;
    }
    const bool thin = fw > 1;
    // ... two of them per SIMD on the principal rows read those rows from the blocks stored with the adjacency, where the index has them
    const bool want_inline = thin && principal_rows && fw == 2u && (knobs.inl >= 0 ? knobs.inl == 1 : kFilterInlinePolicy);
    p.wants_inline = want_inline;
    const bool inlined = want_inline && f.inline_ready;
    p.tab_log2 = tab_log2;
    // the set stores 16-bit quotients (twice the ids in the same LDS) whenever n allows it: up to 33M points with 32 KB
    p.ubits = on_chip ? q16_universe_bits(f.n, tab_log2) : 0u;
    // ... and the walk can outgrow the id form: a search visits ~53 * ef_search + 600 nodes (C3 / C4 / C5 data alike); while that
    // stays below the 7/8 * 2^tab_log2 ids the plain set takes, the plain set never spills and its cheaper probe wins by
    // 1-2 % (ef_search = 100: 10.25 vs 10.42 ms per 10k queries at C3, profiles/r03/probe_r03a_ef_paths_*)
    const bool ids_suffice = 53u * ef + 600u <= (7u << tab_log2) / 8u;
    const bool q16 = on_chip && !knobs.tab_ids && q16_applies(tab_log2, p.ubits) &&
                     (thin || (fat_filtered && !(fat_ids && ids_suffice && !knobs.tab_q16 && !knobs.tab_log2)) || knobs.tab_q16 || knobs.tab_log2 || !ids_suffice);
    // Long walks (ef_search in the hundreds): an expansion costs a wave 9-10 us whatever it fetches, and it fetches fewer new rows
    // the longer the walk runs — more, thinner waves (two 256-register waves per SIMD, as many as the CU's LDS holds) keep more
    // expansions in flight than one fat wave per SIMD.
    // Measured at 300-d (profiles/r04/probe_r04k_ef_paths_two_waves_per_simd_c3.jsonl: ef 650 / 800 / 1000 at 0.704 / 0.690 / 0.651 of
    // spec against 0.653 / 0.639 / 0.628 for the fat waves, 0.787 against 0.795 at ef 400): from ef_search 512 on, for that row
    // geometry; other geometries keep the fat waves until they are measured (IDIST_W2_EF forces either way).
    // Round 5 (profiles/r05/probe_r05r_long_walks_two_waves_other_geometries.jsonl): the same holds for runtime-geometry rows the
    // 256-register tile keeps whole in flight (1M x 384-d: ef 600 / 800 at 79.1 / 105.1 ms against 88.5 / 114.6 ms, ef 400 within
    // 2 %); not for 768-d (fat waves 1 % ahead at ef 400-800) and not for 128-d (thin waves 43 % slower at ef 400).
    const bool w2_geometry = (L.nb == 9 && L.rs == 1 && L.tail == 1) || (rt_rows && L.stride >= 256u && L.nb <= 12u);
    const uint32_t w2_from = knobs.w2_ef != 0xFFFFFFFFu ? knobs.w2_ef : (w2_geometry ? kLongWalkEf : 0xFFFFFFFFu);
    const bool w2 = on_chip && q16 && !quad && !thin && !knobs.classic && ef >= w2_from;
    const uint32_t w2_per_cu = (uint32_t)std::min<size_t>(8, (size_t)160 * 1024 / lds(std::max(tab_log2, 5u)));
    const uint32_t thin_per_cu = (uint32_t)std::min<size_t>(4u * fw, (size_t)160 * 1024 / lds(std::max(tab_log2, 5u), false));
    p.resident = (uint32_t)f.n_cu * (quad ? 2u : (thin ? std::max(thin_per_cu, 4u) : (w2 ? std::max(w2_per_cu, 4u) : (on_chip ? 4u : 16u))));   // quad: two workgroups per CU where registers allow
    // bitmap walk only: narrow batches cannot fill the chip and run its latency variant (same results)
    const bool lat = !on_chip && nq <= knobs.latency_nq && lds((uint32_t)kBloomLatLog2Words) <= 64 * 1024;
    p.smem = lds(on_chip ? tab_log2 : (uint32_t)(lat ? kBloomLatLog2Words : kBloomLog2Words), !thin);
    p.lds_short = p.smem > 64 * 1024;
    const bool principal = thin && principal_rows;
    // (f2 of a principal walk: the identity rows, for the queries the basis does not fit)
    p.filter = principal ? PlanFilter::Principal : (thin || fat_filtered ? PlanFilter::Identity : PlanFilter::None);
    p.inl = inlined;
    p.block = quad ? 256u : 64u;
    // The kernel.  The `classic` walks (one distance round in flight, no adjacency prefetch) are selected by no policy: they exist as
    // independent implementations of the same decisions for the parity tests and are compiled into the TEST build only.
    const bool classic = knobs.classic;
    if (quad && q16) p.walk = SearchWalk::QuadQ16;
    else if (quad) p.walk = SearchWalk::QuadIds;
    else if (thin && principal && fw == 3u) p.walk = SearchWalk::ThinPrincipal3;
    else if (thin && principal && inlined) p.walk = SearchWalk::ThinInline;
    else if (thin && principal) p.walk = SearchWalk::ThinPrincipal;
    else if (thin) p.walk = SearchWalk::ThinIdentity;
    else if (on_chip && classic && q16) p.walk = SearchWalk::ClassicOnChipQ16;
    else if (w2) p.walk = SearchWalk::TwoPerSimd;
    else if (on_chip && fat_filtered && !q16) p.walk = SearchWalk::FatFilteredIds;
    else if (on_chip && fat_filtered) p.walk = SearchWalk::FatFilteredQ16;
    else if (on_chip && q16) p.walk = SearchWalk::OnChipQ16;
    else if (on_chip && classic) p.walk = SearchWalk::ClassicOnChipIds;
    else if (on_chip) p.walk = SearchWalk::OnChipIds;
    else if (lat) p.walk = SearchWalk::Latency;
    else if (classic) p.walk = SearchWalk::ClassicBitmap;
    else p.walk = SearchWalk::OverlapBitmap;
    return p;
}

}  // namespace idist
