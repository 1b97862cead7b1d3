// idist_build_plan.hpp — how a build runs: set, tiles, kernels, streams, and what every step of its schedule launches: the decisions alone.
// plan_build() (once per build) and plan_build_step() (once per step) are pure functions of plain values (BuildFacts, Knobs): no HIP
// call, no index, no allocation, no error path.  run_build (idist_capi.hip) gathers the facts, allocates what the plan sizes and
// launches what each step names; tests/host/build_plan.cpp compiles this header alone and holds the policy against a recorded table
// (tests/golden/build_plan.txt).
#pragma once
#include "idist_search_plan.hpp"
#include "idist_mfma.hpp"

namespace idist {

// Layer sizing of Hnsw::new, core/lib.rs:238-250 (f32 multiply + truncation, `as usize` saturates)
inline uint32_t layer_sizes(uint32_t n, float ml, uint32_t* cum, uint32_t cap) {
    uint32_t cnt = 0;
    size_t num = n;
    for (;;) {
        volatile float prod = (float)num * ml;
        size_t next;
        if (!(prod > 0.0f)) next = 0;
        else if (prod >= 18446744073709551616.0f) next = (size_t)-1;
        else next = (size_t)prod;
        if (next < (size_t)kM) break;
        if (cnt + 1 >= cap) return 0;  // too many layers
        cum[cnt++] = (uint32_t)num;
        num = next;
    }
    cum[cnt++] = (uint32_t)num;
    return cnt;
}

// Everything the policy reads: of the index, of its config, of the attempt (build_common's tie ladder).
struct BuildFacts {
    uint32_t n = 0;
    Layout L{};
    int n_cu = 256;
    uint32_t ef_construction = 0, max_batch = 0;
    bool has_heuristic = false, extend_candidates = false;
    bool metric_l2sq = true;          // the metric the kernels see (kernel_metric) is squared L2
    uint32_t tie_cap = 0;             // the config's tie capacity, resolved (tie_capacity())
    bool tie_spill = false;           // strict ties beyond it go to HBM bags
    bool template_geometry = false;   // has_template_geometry(L)
    bool filter_applies = false;      // filter_applies(n, L)
    uint32_t dirty_words = 0;         // VisGeom::dirty_words of n points
};

// a build that cannot run: some wave needs more than 64 KiB of LDS (run_build words the message)
enum class BuildPlanError : int { None, DescentLds, UpdateTileLds, SelectTileLds, ExtendLds, kCount };
inline const char* build_error_name(BuildPlanError e) {
    static const char* const names[] = {"none", "descent_lds", "update_tile_lds", "select_tile_lds", "extend_lds"};
    static_assert(sizeof(names) / sizeof(names[0]) == (size_t)BuildPlanError::kCount, "one name per error");
    return names[(int)e];
}

// Everything decided once per build.  After an error the fields the rules below had not reached yet keep their defaults.
struct BuildPlan {
    BuildPlanError error = BuildPlanError::None;
    // what the steps' rules read of the facts
    uint32_t n_cu = 256;
    bool ext = false, has_heuristic = false, classic = false;
    // sizes and the descents' on-chip set
    uint32_t cap = 1, slots = 1, wcap = 0;
    uint32_t tab_log2 = 0;
    bool tab16 = false;
    uint32_t ubits = 0, dl_shift = 0, ext_cap = 1;
    // LDS per workgroup: descent, update tile (B2), select tile (A2), extend, Gram select (A2 on MFMA), fast update (B)
    size_t smem = 0, smem_update = 0, smem_select = 0, smem_extend = 0, smem_select_mfma = 0, smem_update_fast = 0;
    size_t tile_budget = 0;           // what the two tiles were first sized for (a tile beyond it fell back to a CU's whole 64 KiB)
    // tiles and kernel choices
    uint32_t fc = 8, rt = 8, rt2 = 16;
    bool a2_mfma = false;
    uint32_t a_waves = 0, a_waves_max = 0;
    bool a_regs256 = false, a_quad = true;
    uint32_t quad_B = 0, growth_div = 8;
    // streams
    bool pipe = false;
    int stream_mode = 1;              // 0 off, 1 narrow steps, 2 all steps on the extra streams
    bool two_a = false, own_a2 = false;
    // flags
    bool use_dlog = true, no_fast = false;
    uint32_t chunk = 0;
    bool wants_filter = false;        // the descents run filtered where the index has the table: make it first (filter_ensure) ...
    bool filtered = false;            // ... and resolve_build_filter() says whether it stands
};
// the filter's final state: the descents run filtered where the policy wants it AND the identity table stands
inline void resolve_build_filter(BuildPlan& p, bool table_ready) { p.filtered = p.wants_filter && table_ready; }

inline BuildPlan plan_build(const BuildFacts& f, const Knobs& knobs) {
    BuildPlan p;
    const uint32_t n = f.n;
    const Layout& L = f.L;
    p.n_cu = (uint32_t)f.n_cu;
    p.has_heuristic = f.has_heuristic;
    p.classic = knobs.classic;
    // a step never holds more than 1/32 of the points already inserted, so scratch is sized by that
    // Heuristic::extend_candidates: defined by the oracle's lock-free restatement (it deadlocks in the reference,
    // core/lib.rs:649 vs :438), one whole insertion per launch in program order — always the sequential schedule
    const bool ext = f.has_heuristic && f.extend_candidates;
    p.ext = ext;
    const uint32_t cap = ext ? 1u : std::min<uint32_t>(f.max_batch == 0 ? 8192u : f.max_batch, std::max<uint32_t>(1u, n / 32u));
    p.cap = cap;
    // the descents keep their visited set on chip, one fat wave per SIMD (up to 8 per CU with the 16-KB quotient set);
    // with the HBM tie bags (one of n keys per slot) as many slots as fit 1 GiB
    uint32_t slots = std::min(cap, (uint32_t)f.n_cu * 8u);
    if (f.tie_spill) slots = std::min<uint32_t>(slots, (uint32_t)std::max<size_t>(1, ((size_t)1 << 30) / ((size_t)n * 8)));
    p.slots = slots;
    // no compile-time instantiation of the row geometry (IDIST_DISPATCH): the runtime-geometry kernels
    const bool rt_geometry = !f.template_geometry;

    const uint32_t wcap = f.ef_construction + 64 + f.tie_cap + 64;
    p.wcap = wcap;
    // The descents' on-chip visited set.  Quotient form (16-bit entries, idist_device.hpp q16_*) where n allows it: 16 KB hold
    // 8192 ids — an ef_construction = 100 descent visits ~6k — so a descent wave takes ~22 KB of LDS instead of ~39 KB
    // and four or five of them leave half the CU's LDS to the update stream.  Otherwise (and IDIST_TAB_FORMAT=ids, ext):
    // full ids, the largest set that leaves room for four waves per CU, or the largest that fits at all.
    uint32_t tab_log2 = 0;
    bool tab16 = false;
    if (!ext && !knobs.tab_ids) {
        const uint32_t want = knobs.tab_log2 ? std::max(8u, std::min(13u, knobs.tab_log2))
                                             : (f.ef_construction <= 128 ? 12u : 13u);
        for (uint32_t l = want; l <= 13 && !tab16; l++)
            if (q16_applies(l, q16_universe_bits(n, l)) && smem_bytes(L.stride, wcap, true, 1u << l, f.dirty_words) <= kOnChipLdsPerWave) {
                tab_log2 = l;
                tab16 = true;
            }
    }
    if (!tab16) {
        for (uint32_t l = 13; l >= 8 && !tab_log2; l--)
            if (smem_bytes(L.stride, wcap, true, 1u << l, f.dirty_words) <= kOnChipLdsPerWave) tab_log2 = l;
        for (uint32_t l = 13; l >= 8 && !tab_log2; l--)
            if (smem_bytes(L.stride, wcap, true, 1u << l, f.dirty_words) <= 64 * 1024) tab_log2 = l;
        if (!tab_log2) { p.error = BuildPlanError::DescentLds; return p; }
        if (knobs.tab_log2) tab_log2 = std::max(8u, std::min(tab_log2, knobs.tab_log2));
    }
    p.tab_log2 = tab_log2;
    p.tab16 = tab16;
    p.ubits = tab16 ? q16_universe_bits(n, tab_log2) : 0u;
    p.dl_shift = tab_log2 + (tab16 ? 1u : 0u);
    const size_t smem = smem_bytes(L.stride, wcap, true, 1u << tab_log2, f.dirty_words);
    p.smem = smem;

    // Tiles of steps B2 / A2 (tile kernel): selected rows kept on chip next to the staging slots.  A tile wave has to find LDS
    // BESIDE the descents of the next step (four waves per CU of `smem` bytes each, resident for a whole launch): a tile that
    // does not fit waits for that launch to drain and the pipeline runs serially — measured at 1024-d, where a 63-KB tile
    // missed the 62 KB left by 1 KB and the full re-selections took 7.4 s of a 9.5-s build.  So: at most what is left of the
    // CU's 160 KiB, at most 64 KiB; long runtime-geometry rows stage four candidates per round instead of eight.
    const bool generic_geo = rt_geometry;
    const size_t lds_beside = (size_t)160 * 1024 > 4 * smem + 8 * 1024 ? (size_t)160 * 1024 - 4 * smem : 8 * 1024;
    const size_t tile_budget = cap > 1 ? std::min<size_t>(64 * 1024, std::max<size_t>(lds_beside, 24 * 1024)) : 64 * 1024;
    p.tile_budget = tile_budget;
    uint32_t fc = 8;
    if (generic_geo && smem_bytes_update(L.nb, 4, 8) > tile_budget) fc = 4;
    uint32_t rt = knobs.build_rt;
    while (rt > 0 && smem_bytes_update(L.nb, rt, fc) > tile_budget) rt--;
    size_t smemB = smem_bytes_update(L.nb, rt, fc);
    if (smemB > tile_budget) {                                   // does not fit beside the descents: take what a CU alone allows
        rt = 8;
        while (rt > 0 && smem_bytes_update(L.nb, rt, fc) > 64 * 1024) rt--;
        smemB = smem_bytes_update(L.nb, rt, fc);
    }
    p.fc = fc;
    p.rt = rt;
    p.smem_update = smemB;
    if (smemB > 64 * 1024) { p.error = BuildPlanError::UpdateTileLds; return p; }

    // step A2 tile: the new point's selected set (up to 64 rows) — it is not memory bound, so favour rows on chip
    uint32_t rt2 = knobs.build_rt2;
    while (rt2 > 0 && smem_bytes_select(L.nb, rt2, f.ef_construction, fc) > tile_budget) rt2--;
    size_t smemA2 = smem_bytes_select(L.nb, rt2, f.ef_construction, fc);
    if (smemA2 > tile_budget) {
        rt2 = 16;
        while (rt2 > 0 && smem_bytes_select(L.nb, rt2, f.ef_construction, fc) > 64 * 1024) rt2--;
        smemA2 = smem_bytes_select(L.nb, rt2, f.ef_construction, fc);
    }
    p.rt2 = rt2;
    p.smem_select = smemA2;
    if (smemA2 > 64 * 1024) { p.error = BuildPlanError::SelectTileLds; return p; }

    uint32_t ext_cap = 1;
    // a selection's working set, padded for the sort: nearest (<= ef_construction for the new point, <= 65 = new + a full
    // row for a neighbour's re-selection, whatever ef_construction is) plus up to 64 extensions per member
    while (ext_cap < (std::max(f.ef_construction, 65u) + 1u) * 65u + 64u) ext_cap <<= 1;
    p.ext_cap = ext_cap;
    p.smem_extend = smem_bytes_extend(L.stride, wcap, 1u << tab_log2, f.dirty_words);
    if (ext && p.smem_extend > 64 * 1024) { p.error = BuildPlanError::ExtendLds; return p; }
    // step A2 on the matrix cores (Gram matrix of the candidates as a filter, idist_mfma.hpp) where it applies
    p.a2_mfma = f.has_heuristic && f.metric_l2sq && f.ef_construction <= 128 && !knobs.build_a2_tile;
    p.smem_select_mfma = smem_bytes_select_mfma(L.stride);
    // Pipelined schedule (default for concurrent builds with the heuristic): the descents of step k+1 (HBM-bound)
    // run on one stream while the selections / neighbour updates of step k (LDS- and latency-bound) run on another.
    // Step k's descents read the graph as of step k-2, so nothing they read is being written: the zero layer is
    // kept in two copies, copy k&1 receiving the state after step k.  Deterministic like the sequential schedule;
    // a new point then misses the last two steps' points (<= 1/16 of the graph) instead of the last one's.
    bool pipe = cap > 1 && f.has_heuristic;
    pipe = pipe && knobs.build_pipeline;
    p.pipe = pipe;
    // the descents (8-12 waves per CU saturate their HBM stream) leave wave slots and LDS to the other stream
    uint32_t a_waves = tab16 ? 4u : 3u;
    if (knobs.build_a_waves) a_waves = knobs.build_a_waves;
    // the descent's register budget (quotient set only): 256 registers per wave (two waves fit a SIMD: the update stream's
    // waves find room on every SIMD) or 512 (IDIST_BUILD_A_REGS=512, more rounds in flight per wave).  C3: 1.26 vs 1.29-1.32 s
    // Runtime-geometry rows (any dimension without a compile-time instantiation): the register tile, not the row, bounds what a
    // wave keeps on the wire, and the 256-register tile (2 x 3 rounds x 4 blocks = 24 KB) is too little at four waves per
    // CU: one 512-register wave per SIMD (2 x 4 x 8 = 64 KB each) builds 1M x 1024-d in 4.35 s instead of 9.6 s and 1M x 384-d
    // in 1.98 s instead of 2.66 s (profiles/r04/probe_r04d_build_dim*.jsonl) although the update stream then only runs where a
    // descent wave has retired.
    // Which register budget the descents take (same graphs either way; round 5):
    //   * the 128-d instantiation (4 blocks): one fat wave per SIMD at EVERY size — C2 100k x 128: 0.110 against 0.121 s (five to
    //     eight thin waves per CU: 0.117-0.122 s); 300k / 600k / 1M x 128: 0.245 / 0.449 / 0.713 s against 0.286 / 0.550 / 0.915 s
    //     (profiles/r05/probe_r05c_build_descent_waves_c2.jsonl, probe_r05p_build_regs_mid_size_short_rows.jsonl);
    //   * 300-d and 768-d rows: two 256-register waves per SIMD, also where the index sits in the Infinity Cache (C3 1.26 against
    //     1.29-1.32 s, C4 2.78-2.83 against 3.00-3.06 s; 40k x 768: 0.139 against 0.153 s; 60k-200k x 300: within 2 %,
    //     probe_r05q_build_regs_cache_resident_long_rows.jsonl);
    //   * runtime-geometry rows of at most 12 blocks (<= 384-d) fit the 256-register tile whole (<6 blocks, 3 rounds>, two groups in
    //     flight) and build faster on it — 1M x 64 / 100 / 200 / 384-d: 0.91 / 1.11 / 1.30 / 1.75 s against 1.18 / 1.38 / 1.55 / 1.96 s;
    //     longer rows keep the fat waves (512-d: 2.35 against 3.12 s, 500k x 1024-d: 2.26 against 4.19 s; probe_r05g_*, probe_r05p_*).
    const bool rows128 = L.nb == 4 && L.rs == 0 && L.tail == 0;
    bool a_regs256 = tab16 && !rows128 && (!rt_geometry || L.nb <= 12u);
    if (knobs.build_a_regs >= 0) a_regs256 = tab16 && knobs.build_a_regs == 256;
    p.a_regs256 = a_regs256;
    // (Fat descent waves take a SIMD's whole register file: where four of them sit on a CU, nothing of the update stream runs until
    //  one retires — at 1024-d the selection's launches stretch to the descents' 13 ms and a step's period is 16.5 ms for 12.9 ms of
    //  descents, profiles/r05/trace_chain_r05i_build_500k_dim1024.json.  Measured and not kept: fewer descent waves per step, so that some
    //  SIMDs stay free — 960 / 896 / 768 waves build 500k x 1024-d in 2.25 / 2.31 / 2.51 s against 2.20 s, probe_r05j; the update
    //  streams at the highest priority — no difference at 1024 / 512 / 768 / 300-d, probe_r05k.)
    // steps of at most two insertions per CU run four waves per insertion (IDIST_BUILD_QUAD=0: never)
    p.a_quad = knobs.build_quad;
    p.quad_B = (uint32_t)f.n_cu * 2u;
    // Narrow steps (four waves per insertion: their time does not depend on their width — one descent ≈ 0.45 ms) hold g / 8
    // insertions until they stop being narrow, wide ones g / 32: the first 16k points of a build take ≈ 60 steps instead of
    // ≈ 180 (100k x 128: 0.156 -> 0.122 s, 20k x 128: 0.078 -> 0.043 s, C3 -2.6 %; recall@10 unchanged to the fourth digit at
    // 5k / 20k / 100k / 1M points, profiles/r04/probe_r04_build_growth_*.jsonl).  IDIST_BUILD_GROWTH=<d> (A/B knob, 8..32): g / d.
    p.growth_div = knobs.build_growth;
    // what one CU's LDS holds of them (the sequential schedule runs nothing beside the descents)
    p.a_waves_max = std::max<uint32_t>(1u, std::min<uint32_t>(8u, (uint32_t)((160u * 1024u) / smem)));
    p.a_waves = std::min(a_waves, p.a_waves_max);
    // Narrow steps (the growth phase of every layer: fewer insertions than the chip has room for) are bound by the latency of
    // one descent plus five dependent launches, not by throughput, so there the two parity chains of the pipeline
    //     descents(k) -> selection(k) -> updates(k) -> descents(k + 2)
    // get streams of their own: the descents of odd steps (s3) run beside those of even steps (s1), and the new points'
    // selection (s4: matrix cores and LDS) beside the previous step's neighbour updates (s2: dependent gathers).  Everything
    // a launch owns is kept per parity for that — visited bitmaps, work-queue heads, step-A outputs, the inboxes the selection
    // hands to the updates.  Wide steps saturate the memory system whatever the layout (profiles/r04/probe_r04_build_schedule:
    // the extra overlap costs 2 %), so they keep one descent stream and one update stream.
    // IDIST_BUILD_STREAMS=off | narrow (default) | all.
    p.stream_mode = knobs.build_streams;
    p.two_a = !f.tie_spill && p.stream_mode != 0 && pipe;
    p.own_a2 = p.stream_mode != 0 && pipe;

    // Round 6: the descents of concurrent steps run with the reject filter in front of their distance passes (§4.5) — the compact
    // copy of the rows is made now (every row is in place before the first insertion), the log takes bound-form entries for the
    // candidates the filter turned down, step B resolves them (dlog_resolve).  IDIST_BUILD_FILTER=0 (test knob): without.
    // Rows of at least 192 floats: C3 1.20 -> 1.03 s, 1M x 768 2.82 -> 2.01 s, 1M x 384 1.71 -> 1.29 s, 1M x 200 1.22 -> 1.12 s
    // (probe_r06v_build_filter_128_recheck.jsonl); 128-d rows lose (a 192-B compact
    // row saves little of a 512-B one and their fat unfiltered descents are faster: 1M x 128 0.70 -> 0.85 s, C2 0.107 -> 0.118 s) and
    // keep the unfiltered descents (profiles/probe_r06g_build_filter_c3.jsonl, probe_r06h_build_filter_dims.jsonl; same graphs).
    // IDIST_BUILD_FILTER=1 (test knob) forces it for every geometry the filter applies to.
    p.wants_filter = f.has_heuristic && !ext && tab16 && knobs.filter && f.filter_applies &&
                     (f.template_geometry || filt_stride(L.stride) <= 128u * (uint32_t)kFiltRtChunks) &&   // (the thin tile)
                     (knobs.build_filter >= 0 ? knobs.build_filter != 0 : L.stride >= 192u);
    // (fat filtered descents for runtime-geometry rows beyond the thin tile: 500k x 1024 / 1536-d 2.04 / 2.78 against 2.10 / 3.13 s —
    //  profiles/probe_r06r_build_fat_filtered_1024.jsonl — not worth their compile time: those descents stay unfiltered)
    // (one FAT filtered descent wave per SIMD, the search's layout for 768-d rows, builds 1M x 768 in 2.56 s against 2.37 s on the thin
    //  ones: the update stream needs the registers — profiles/probe_r06n_build_fat_768.jsonl)
    p.use_dlog = knobs.build_dlog;
    p.chunk = knobs.build_chunk;
    p.no_fast = knobs.build_no_fast;
    p.smem_update_fast = smem_bytes_update_fast(L.stride);
    return p;
}

// one value per descent kernel of a step, in the order the rules of plan_build_step test them
enum class BuildDescent : int {
    Extend,                           // extend_candidates: one whole insertion per launch
    ClassicQ16, ClassicIds,           // (test builds)
    FourWaveQ16,                      // narrow steps: four waves per insertion
    ThinFiltered,
    TwoPerSimd,
    FatQ16, FatIds,
    kCount
};
inline const char* descent_name(BuildDescent d) {
    static const char* const names[] = {"extend", "classic_q16", "classic_ids", "four_wave_q16", "thin_filtered", "two_per_simd", "fat_q16", "fat_ids"};
    static_assert(sizeof(names) / sizeof(names[0]) == (size_t)BuildDescent::kCount, "one name per descent");
    return names[(int)d];
}
// The streams of a pipelined build by what they carry (run_build maps the roles to its streams; a build that is not pipelined has
// one stream for all of them).  The updates of a step always run on the update stream.
enum class DescentStream : int { Descent0, Descent1, Update };   // the descents of a step: s1, s3 (odd narrow steps), or behind the updates (sequential steps)
enum class SelectStream : int { Update, Selection };             // the new points' selection: ahead of the updates on their stream, or on its own (s4)

struct BuildStep {
    uint32_t B = 1;                   // insertions this step holds
    int par = 0;                      // k & 1: which copy of the zero layer receives the state after this step, which set of per-parity buffers it owns
    bool alt = false;                 // narrow: this step on the extra streams
    bool seq1 = false;                // sequential: all of its launches on the update stream
    int lag = 0;                      // pipelined: the descents read the state after step k - lag (0: not pipelined)
    BuildDescent descent = BuildDescent::FatIds;
    uint32_t gridA = 0, gridB = 0, gridS = 0, gridA2 = 0, gridA2m = 0;
    DescentStream descent_stream = DescentStream::Descent0;
    SelectStream select_stream = SelectStream::Update;
};

// Step k (1-based) of a build: the insertions [g, g + B) of `layer`, whose points end at `end`.
inline BuildStep plan_build_step(const BuildPlan& p, uint32_t top, uint32_t layer, uint32_t g, uint32_t end, uint64_t k, bool first_of_layer) {
    BuildStep s;
    // top layer is sequential in the reference (:313-314); below, at most `cap` inserts run
    // concurrently (:316-318) and never more than 1/32 of the graph they search (1/8 while the step is narrow).
    uint32_t B = 1;
    if (p.cap > 1 && layer != top && g >= 64) B = std::min(p.cap, std::max(std::min(g / p.growth_div, p.quad_B), g / 32u));
    B = std::min(B, end - g);
    s.B = B;
    s.par = (int)(k & 1u);
    s.alt = p.stream_mode == 2 || (p.stream_mode == 1 && B <= p.quad_B);   // this step on the extra streams
    // a sequential step (B = 1: the top layer, the first 63 points) depends on the whole previous step anyway: all of its
    // launches go to the update stream — same-stream boundaries (~2 us) instead of three cross-stream event hops (~27 us each
    // in the trace of profiles/r05/trace_chain_r05b_build_c2.json: 74 of the 179 us such a step took)
    // Only where every descent stream has its own queue head, visited bitmaps and tie bags (two_a): with ONE set of them (a build
    // on the HBM tie bags, IDIST_BUILD_STREAMS=off) the last sequential step's descent on s2 and the next, concurrent step's
    // descent on s1 — which waits for the step BEFORE it only — would share them.
    s.seq1 = p.pipe && p.two_a && B == 1;
    s.descent_stream = s.seq1 ? DescentStream::Update : (p.pipe && p.two_a && s.alt && s.par ? DescentStream::Descent1 : DescentStream::Descent0);
    s.select_stream = p.pipe && p.own_a2 && s.alt && !s.seq1 ? SelectStream::Selection : SelectStream::Update;
    // a sequential (B = 1) step reads the previous step's state, a concurrent one the state before that.
    // The first step of a layer reads the previous step's state too: the snapshot of the layer above was
    // taken from it (s1 has waited for it already), and a descent that enters the zero layer through a
    // node of that last step must find its row, not the all-INVALID one of the older copy.
    s.lag = p.pipe ? (B > 1 && !first_of_layer ? 2 : 1) : 0;
    s.gridA = std::min(B, std::min<uint32_t>(p.slots, p.n_cu * (p.pipe ? p.a_waves : std::min(p.a_waves_max, p.a_regs256 ? 8u : 4u))));
    s.gridB = (uint32_t)std::min<size_t>(std::min<size_t>((size_t)B * kM2, g), (size_t)p.n_cu * 16);
    s.gridS = std::min<uint32_t>(s.gridB, p.n_cu * 6);
    s.gridA2 = std::min<uint32_t>(B, p.n_cu * 4);
    s.gridA2m = std::min<uint32_t>(B, p.n_cu * 2);
    // The descents' kernel.  The `classic` walks are selected by no policy (test builds only, see plan_search).
    if (p.ext) s.descent = BuildDescent::Extend;
    else if (p.classic && p.tab16) s.descent = BuildDescent::ClassicQ16;
    else if (p.classic) s.descent = BuildDescent::ClassicIds;
    // narrow steps (the growth phase of a layer, max_batch = 1): four waves per insertion, like narrow search batches
    else if (p.tab16 && p.a_quad && B <= p.quad_B) s.descent = BuildDescent::FourWaveQ16;
    // ... and with the reject filter in front of the distance passes (thin: one f32 round in flight, query fragment from LDS)
    else if (p.tab16 && p.filtered) s.descent = BuildDescent::ThinFiltered;
    // two descent waves per SIMD: 256 registers each, fewer rounds in flight per wave, more waves
    else if (p.tab16 && p.a_regs256) s.descent = BuildDescent::TwoPerSimd;
    else if (p.tab16) s.descent = BuildDescent::FatQ16;
    else s.descent = BuildDescent::FatIds;
    return s;
}

}  // namespace idist
