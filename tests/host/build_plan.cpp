// plan_build / plan_build_step alone (instant-distance_amd/csrc/idist_build_plan.hpp): set, tiles, kernels and streams of a build and
// what every step of its schedule launches, as pure functions of plain values — on the CPU, no device.  Compiled and run by
// tests/test_build_plan.py.
//   build_plan check TABLE   every line of tests/golden/build_plan.txt (facts and knobs -> the plan, the number of steps, a digest of
//                            the steps; RECORDED from run_build as it was before the policy became these functions) against them, byte
//                            for byte; the table must hold the cases its header lists; then the properties below over the full cross
//                            product of the lists
//   build_plan print [full]  the table's lines (full: the cross product's) as the plan gives them: an intended policy change is the
//                            diff of this output against the committed file
//   build_plan cases [full]  the same cases, facts and knobs only (what a recorder of run_build's own decisions reads)
//   build_plan steps CASE... the steps of one case (its eight input fields), one line each
// A line: `dim n efc max_batch selection tie_spill tie_cap knob -> PLAN | n_steps | digest`, at 256 CUs, layers by layer_sizes(n, 1 / ln 32);
// PLAN: `cap slots wcap tab_log2 tab16 ubits dl_shift ext_cap | LDS: descent update select extend gram_select fast_update |
//        fc rt rt2 a2_mfma a_waves a_waves_max a_regs256 a_quad quad_B growth_div | pipe stream_mode two_a own_a2 | use_dlog no_fast chunk |
//        wants_filter`, or `error NAME [bytes]`.
// The digest is FNV-1a (64 bit) over the steps' tuples `layer g B par alt seq1 lag descent gridA gridB gridS gridA2 gridA2m
// descent-stream selection-stream`, each value as eight little-endian bytes, with the filter table taken as made.  Once a layer's steps
// have reached their full width (B == cap: one insertion per step at max_batch = 1, 10 M steps of four at max_batch = 4 and 40 M points)
// they repeat but for g and the parity: from a layer's 257th step on, a run of full-width steps is counted, not walked, up to the last
// two full steps of the layer (and what is left after them) — the recording skipped the same runs.  Nothing a step decides changes inside
// such a run: every rule of plan_build_step reads g only through B (== cap throughout: B does not shrink while g grows, but in the
// layer's tail, which is walked) and through gridB = min(64 * B, g, 16 * n_cu), which does not shrink while g grows either;
// first_of_layer is off, and the parity is k & 1, which the count keeps.  So a run whose two ends agree agrees throughout, and `check`
// asserts over the full product that the step in front of every counted run and the step behind it are equal in everything but g and
// what follows the parity.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../instant-distance_amd/csrc/idist_build_plan.hpp"

using namespace idist;

static const uint32_t kCus = 256;
static const uint32_t kMaxLayers = 32;
static const char* const kSelNames[] = {"simple", "heuristic", "extend"};
struct Case {
    uint32_t dim = 0, n = 0, efc = 0, max_batch = 0;
    int sel = 1;
    uint32_t tie_spill = 0, tie_cap = (uint32_t)kTieCap;
    std::string knob = "default";
};
// `default`, or the test knobs that are set: Knobs' field names, joined by commas
static bool knob_of(const std::string& tok, Knobs& k) {
    char name[32];
    unsigned v;
    if (sscanf(tok.c_str(), "%31[a-z0-9_]=%u", name, &v) != 2) return false;
    const std::string nm = name;
    if (nm == "classic") k.classic = v;
    else if (nm == "tab_log2") k.tab_log2 = v;
    else if (nm == "tab_ids") k.tab_ids = v;
    else if (nm == "build_rt") k.build_rt = v;
    else if (nm == "build_rt2") k.build_rt2 = v;
    else if (nm == "build_a2_tile") k.build_a2_tile = v;
    else if (nm == "build_pipeline") k.build_pipeline = v;
    else if (nm == "build_a_waves") k.build_a_waves = v;
    else if (nm == "build_a_regs") k.build_a_regs = (int)v;
    else if (nm == "build_quad") k.build_quad = v;
    else if (nm == "build_growth") k.build_growth = v;
    else if (nm == "build_streams") k.build_streams = (int)v;
    else if (nm == "build_filter") k.build_filter = (int)v;
    else if (nm == "build_dlog") k.build_dlog = v;
    else if (nm == "build_chunk") k.build_chunk = v;
    else if (nm == "build_no_fast") k.build_no_fast = v;
    else return false;
    return true;
}
static bool knobs_of(const std::string& toks, Knobs& k) {
    if (toks == "default") return true;
    size_t pos = 0;
    while (pos <= toks.size()) {
        size_t c = toks.find(',', pos);
        if (c == std::string::npos) c = toks.size();
        if (!knob_of(toks.substr(pos, c - pos), k)) return false;
        pos = c + 1;
    }
    return true;
}
static std::string fmt_inputs(const Case& c) {
    char buf[200];
    snprintf(buf, sizeof(buf), "%u %u %u %u %s %u %u %s", c.dim, c.n, c.efc, c.max_batch, kSelNames[c.sel], c.tie_spill, c.tie_cap, c.knob.c_str());
    return buf;
}
static bool parse_inputs(const char* line, Case& c) {
    char sel[16], knob[128];
    if (sscanf(line, "%u %u %u %u %15s %u %u %127s", &c.dim, &c.n, &c.efc, &c.max_batch, sel, &c.tie_spill, &c.tie_cap, knob) != 8) return false;
    c.knob = knob;
    for (c.sel = 0; c.sel < 3 && strcmp(sel, kSelNames[c.sel]); c.sel++) {}
    Knobs k;
    return c.sel < 3 && knobs_of(c.knob, k);
}
static BuildFacts facts_of(const Case& c) {
    BuildFacts f;
    f.n = c.n;
    f.L = make_layout(c.dim);
    f.n_cu = (int)kCus;
    f.ef_construction = c.efc;
    f.max_batch = c.max_batch;
    f.has_heuristic = c.sel >= 1;
    f.extend_candidates = c.sel == 2;
    f.metric_l2sq = true;
    f.tie_cap = c.tie_cap;
    f.tie_spill = c.tie_spill != 0;
    f.template_geometry = has_template_geometry(f.L);
    f.filter_applies = filter_applies(f.n, f.L);
    f.dirty_words = vis_geometry(c.n).dirty_words;
    return f;
}
static BuildPlan plan_of(const Case& c) {
    Knobs k;
    knobs_of(c.knob, k);
    BuildPlan p = plan_build(facts_of(c), k);
    resolve_build_filter(p, true);      // (the table's steps: with the filter table made)
    return p;
}

// ---- the schedule of a build (run_build's loops), every step handed to `visit`; false from `visit` ends the walk
constexpr uint32_t kHeadSteps = 256, kTailSteps = 2;    // what of a layer is walked whatever its steps' width (see the head of this file)
template <class F> static uint64_t walk_steps(const Case& c, const BuildPlan& p, F visit) {
    uint32_t cum[kMaxLayers + 1];
    const uint32_t nl = layer_sizes(c.n, 1.0f / logf((float)kM), cum, kMaxLayers);
    if (c.n <= 1 || nl == 0) return 0;                   // pid 0 is never inserted
    const uint32_t top = nl - 1;
    uint64_t k = 0;
    for (int layer = (int)top; layer >= 0; layer--) {
        const uint32_t end = cum[layer];
        uint32_t g = (uint32_t)layer == top ? 1u : std::max(cum[layer + 1], 1u);
        bool first = true;
        uint32_t in_layer = 0, prev_B = 0;
        while (g < end) {
            if (in_layer >= kHeadSteps && prev_B == p.cap && (end - g) / p.cap > kTailSteps) {
                const uint32_t skip = (end - g) / p.cap - kTailSteps;
                g += skip * p.cap;
                k += skip;
            }
            in_layer++;
            const BuildStep s = plan_build_step(p, top, (uint32_t)layer, g, end, k + 1, first);
            if (!visit(layer, g, end, k + 1, first, s)) return k;
            prev_B = s.B;
            g += s.B;
            k++;
            first = false;
        }
    }
    return k;
}
static std::string fmt_step(int layer, uint32_t g, const BuildStep& s) {
    char buf[200];
    snprintf(buf, sizeof(buf), "%d %u %u %d %d %d %d %s %u %u %u %u %u %d %d", layer, g, s.B, s.par, (int)s.alt, (int)s.seq1, s.lag, descent_name(s.descent),
             s.gridA, s.gridB, s.gridS, s.gridA2, s.gridA2m, (int)s.descent_stream, (int)s.select_stream);
    return buf;
}
struct Digest {
    uint64_t h = 14695981039346656037ull;
    void put(uint64_t v) { for (int i = 0; i < 8; i++) { h ^= (v >> (8 * i)) & 0xFFull; h *= 1099511628211ull; } }
};

// the plan: see the head of this file
static std::string fmt_plan(const Case& c, const BuildPlan& p, std::set<std::string>* seen = nullptr, bool steps_too = true) {
    char buf[512];
    if (p.error != BuildPlanError::None) {
        const size_t bytes = p.error == BuildPlanError::UpdateTileLds ? p.smem_update : (p.error == BuildPlanError::SelectTileLds ? p.smem_select : p.smem_extend);
        if (p.error == BuildPlanError::DescentLds) snprintf(buf, sizeof(buf), "error %s", build_error_name(p.error));
        else snprintf(buf, sizeof(buf), "error %s %zu", build_error_name(p.error), bytes);
        return buf;
    }
    snprintf(buf, sizeof(buf), "%u %u %u %u %d %u %u %u | %zu %zu %zu %zu %zu %zu | %u %u %u %d %u %u %d %d %u %u | %d %d %d %d | %u %d %u | %s",
             p.cap, p.slots, p.wcap, p.tab_log2, (int)p.tab16, p.ubits, p.dl_shift, p.ext_cap, p.smem, p.smem_update, p.smem_select, p.smem_extend,
             p.smem_select_mfma, p.smem_update_fast, p.fc, p.rt, p.rt2, (int)p.a2_mfma, p.a_waves, p.a_waves_max, (int)p.a_regs256, (int)p.a_quad,
             p.quad_B, p.growth_div, (int)p.pipe, p.stream_mode, (int)p.two_a, (int)p.own_a2, p.use_dlog ? 1u : 0u, (int)p.no_fast, p.chunk,
             p.wants_filter ? "filter" : "-");
    if (!steps_too) return buf;
    Digest d;
    const uint64_t steps = walk_steps(c, p, [&](int layer, uint32_t g, uint32_t, uint64_t, bool first, const BuildStep& s) {
        const uint64_t t[15] = {(uint64_t)layer, g, s.B, (uint64_t)s.par, s.alt, s.seq1, (uint64_t)s.lag, (uint64_t)s.descent, s.gridA, s.gridB, s.gridS,
                                s.gridA2, s.gridA2m, (uint64_t)s.descent_stream, (uint64_t)s.select_stream};
        for (uint64_t v : t) d.put(v);
        if (seen) {
            seen->insert(std::string("descent=") + descent_name(s.descent));
            if (first && s.B > 1 && s.lag == 1) seen->insert("first_of_layer_lag1");
        }
        return true;
    });
    char tail[64];
    snprintf(tail, sizeof(tail), " | %" PRIu64 " | %016" PRIx64, steps, d.h);
    return std::string(buf) + tail;
}
static const char* const kHeader =
    "# dim n efc max_batch selection tie_spill tie_cap knob -> cap slots wcap tab_log2 tab16 ubits dl_shift ext_cap | descent update select extend "
    "gram_select fast_update (LDS) | fc rt rt2 a2_mfma a_waves a_waves_max a_regs256 a_quad quad_B growth_div | pipe stream_mode two_a own_a2 | "
    "use_dlog no_fast chunk | wants_filter | n_steps | digest of the steps\n"
    "# (or `-> error NAME [bytes]`).  tie_spill on comes at the default tie capacity (the test knob IDIST_TIE_SPILL=1) and at 4096, where the\n"
    "# build's own ladder turns to the bags.  Of the four errors the recording reaches extend_lds only (every extend_candidates build at tie\n"
    "# capacity 4096; none at the default capacity).  The other three need more than the lists' largest case has: at 1536-d, ef_construction\n"
    "# IDIST_MAX_EF and tie capacity 4096 the descent takes 63,840 B with a set of 2^11 ids, the update tile 60,672 B with five rows\n"
    "# on chip and the select tile 64,576 B with four — all within 65,536 B.";
static std::string fmt_line(const Case& c, std::set<std::string>* seen = nullptr) { return fmt_inputs(c) + " -> " + fmt_plan(c, plan_of(c), seen); }

// ---- the lists (the issue's)
static const uint32_t kDims[] = {64, 100, 128, 200, 300, 384, 512, 768, 1024, 1536};
static const uint32_t kNs[] = {2u, 63u, 64u, 1000u, 20000u, 100000u, 1000000u, 10000000u, 40000000u};   // the last: beyond the quotient form's reach
static const uint32_t kEfcs[] = {16, 100, 128, 129, 400, 1536};                                         // the last: IDIST_MAX_EF
static const uint32_t kMaxBatches[] = {0, 1, 4};
static const uint32_t kTieMax = 4096;       // what build_common's ladder reaches before it turns to the HBM bags
// tie_spill off; on at the default capacity (IDIST_TIE_SPILL=1) and at the ladder's last rung
static const struct { uint32_t spill, cap; } kTies[] = {{0, (uint32_t)kTieCap}, {1, (uint32_t)kTieCap}, {1, kTieMax}};
// the default knobs, each build knob alone at each value a test or tests/parity_cases.py uses, each pair parity_cases.BUILD_VARIANTS sets together
static const char* const kKnobSets[] = {"default", "build_quad=0", "build_filter=0", "build_filter=1", "build_a_regs=512", "build_a_regs=256", "build_a2_tile=1",
                                        "build_pipeline=0", "build_streams=0", "build_streams=2", "build_growth=32", "build_a_waves=8", "build_rt=2",
                                        "build_rt2=4", "build_no_fast=1", "build_dlog=0", "build_chunk=5", "tab_log2=7", "tab_ids=1", "classic=1",
                                        "build_quad=0,build_filter=1", "build_quad=0,build_filter=0", "build_quad=0,build_a_regs=512",
                                        "build_a2_tile=1,build_no_fast=1", "tab_ids=1,tab_log2=7", "tab_log2=5,classic=1"};
static Case make_case(uint32_t dim, uint32_t n, uint32_t efc, uint32_t mb, int sel, const char* knob = "default", uint32_t spill = 0, uint32_t tie_cap = (uint32_t)kTieCap) {
    Case c;
    c.dim = dim; c.n = n; c.efc = efc; c.max_batch = mb; c.sel = sel; c.knob = knob; c.tie_spill = spill; c.tie_cap = tie_cap;
    return c;
}
template <class F> static void full_cases(F emit) {
    for (uint32_t dim : kDims) for (uint32_t n : kNs) for (uint32_t efc : kEfcs) for (uint32_t mb : kMaxBatches) for (int sel = 0; sel < 3; sel++)
        for (auto t : kTies) for (const char* k : kKnobSets) emit(make_case(dim, n, efc, mb, sel, k, t.spill, t.cap));
}
// The committed table: a selection of the cross product (every line of it is one of full_cases').
template <class F> static void table_cases(F emit_raw) {
    std::set<std::string> seen;
    auto emit = [&](const Case& c) { if (seen.insert(fmt_inputs(c)).second) emit_raw(c); };
    // every geometry, from two points to beyond the quotient form, concurrent and sequential, at the default ef_construction
    for (uint32_t dim : kDims) for (uint32_t n : kNs) for (uint32_t mb : {0u, 1u}) emit(make_case(dim, n, 100, mb, 1));
    // the geometries with kernels of their own, a short and a long runtime one: every ef_construction, every selection, every tie state
    for (uint32_t dim : {64u, 128u, 300u, 768u, 1024u}) {
        for (uint32_t efc : kEfcs) for (int sel = 0; sel < 3; sel++) emit(make_case(dim, 1000000, efc, 0, sel));
        for (auto t : kTies) for (uint32_t n : {20000u, 40000000u}) emit(make_case(dim, n, 100, 0, 1, "default", t.spill, t.cap));
    }
    // each knob set
    for (const char* k : kKnobSets) for (uint32_t dim : {128u, 300u, 1024u}) for (uint32_t n : {20000u, 1000000u}) emit(make_case(dim, n, 100, 0, 1, k));
    for (const char* k : {"build_streams=0", "build_streams=2", "build_pipeline=0", "classic=1", "tab_ids=1"}) {
        emit(make_case(300, 100000, 100, 4, 1, k));
        emit(make_case(300, 100000, 100, 0, 0, k));
        emit(make_case(300, 100000, 100, 0, 1, k, 1, kTieMax));
    }
    // tiles that do not fit beside the descents, and waves that do not fit at all
    for (uint32_t dim : {512u, 768u, 1024u, 1536u}) for (uint32_t efc : {400u, 1536u}) for (auto t : kTies) for (int sel : {1, 2})
        emit(make_case(dim, 1000000, efc, 0, sel, "default", t.spill, t.cap));
}

// ---- properties of every plan and of its steps
static const char* broken_property(const Case& c) {
    const BuildPlan p = plan_of(c);
    if (fmt_plan(c, p, nullptr, false) != fmt_plan(c, plan_of(c), nullptr, false)) return "planning twice from the same facts gives two plans";
    if (p.slots < 1) return "no descent slot";
    if (p.error != BuildPlanError::None) return nullptr;
    for (size_t b : {p.smem, p.smem_update, p.smem_select, p.smem_select_mfma, p.smem_update_fast})
        if (b > 64 * 1024) return "an LDS size beyond 64 KiB in a plan without an error";
    if (p.ext && p.smem_extend > 64 * 1024) return "the extend kernel's LDS beyond 64 KiB in a plan without an error";
    if (p.two_a && !p.pipe) return "two descent streams without the pipeline";
    if (p.tab16 && !q16_applies(p.tab_log2, p.ubits)) return "the quotient form where it does not apply";
    uint32_t cum[kMaxLayers + 1];
    const uint32_t nl = layer_sizes(c.n, 1.0f / logf((float)kM), cum, kMaxLayers);
    const uint32_t top = nl - 1;
    const char* what = nullptr;
    int cur_layer = -1;
    uint32_t expect_g = 0, last_end = 0;
    uint64_t expect_k = 1;
    BuildStep prev;
    walk_steps(c, p, [&](int layer, uint32_t g, uint32_t end, uint64_t k, bool first, const BuildStep& s) {
        if (layer != cur_layer) {
            if (cur_layer >= 0 && expect_g != last_end) what = "the steps of a layer do not end at its end";
            if (!first) what = "a layer's first step is not marked";
            if (g != ((uint32_t)layer == top ? 1u : std::max(cum[layer + 1], 1u))) what = "a layer's first step does not start at its start";
            cur_layer = layer;
        } else {
            const bool skipped = g > expect_g && (g - expect_g) % p.cap == 0 && k - expect_k == (g - expect_g) / p.cap &&
                                 (end - g) / p.cap == kTailSteps;                                            // (walk_steps' counted run)
            if (g != expect_g && !skipped) what = "the steps of a layer leave a gap or overlap";
            if (k != expect_k && !skipped) what = "the steps are not numbered in order";
            // (the descent stream follows alt, seq1 and the parity)
            if (skipped && !(s.B == prev.B && s.B == p.cap && s.alt == prev.alt && s.seq1 == prev.seq1 && s.lag == prev.lag && s.descent == prev.descent &&
                             s.gridA == prev.gridA && s.gridB == prev.gridB && s.gridS == prev.gridS && s.gridA2 == prev.gridA2 &&
                             s.gridA2m == prev.gridA2m && s.select_stream == prev.select_stream))
                what = "the steps at the two ends of a counted run differ in more than g and the parity";
        }
        prev = s;
        if (s.B < 1 || s.B > end - g) what = "a step beyond its layer's end";
        if (((uint32_t)layer == top || g < 64) && s.B != 1) what = "a concurrent step on the top layer or below 64 points";
        if (s.B > p.cap) what = "a step wider than cap";
        if (s.B > p.quad_B && s.B > std::max(g / 32u, 1u)) what = "a wide step of more than 1/32 of the points it searches";
        if (s.seq1 && !p.two_a) what = "a sequential step on the update stream without two descent streams' own buffers";
        if (s.par != (int)(k & 1u)) what = "par != k & 1";
        if ((s.lag == 0) != !p.pipe || s.lag > 2) what = "lag outside 1..2 in a pipelined build (or set in another)";
        if (s.gridA < 1 || s.gridA > p.slots) what = "more descent workgroups than slots (or none)";
        if (s.descent_stream == DescentStream::Descent1 && !p.two_a) what = "the second descent stream where there is none";
        if (s.select_stream == SelectStream::Selection && !p.own_a2) what = "the selection stream where there is none";
        if ((s.descent == BuildDescent::ClassicQ16 || s.descent == BuildDescent::ClassicIds) != (p.classic && !p.ext)) what = "a classic descent without the knob (or the reverse)";
        expect_g = g + s.B;
        expect_k = k + 1;
        last_end = end;
        return what == nullptr;
    });
    if (!what && cur_layer >= 0 && expect_g != last_end) what = "the steps of the zero layer do not end at n";
    return what;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    const bool full = argc > 2 && !strcmp(argv[2], "full");
    if (mode == "print" || mode == "cases") {
        auto emit = [&](const Case& c) { puts((mode == "print" ? fmt_line(c) : fmt_inputs(c)).c_str()); };
        if (mode == "print" && !full) puts(kHeader);
        if (full) full_cases(emit); else table_cases(emit);
        return 0;
    }
    if (mode == "steps" && argc > 2) {
        std::string in;
        for (int i = 2; i < argc; i++) in += std::string(i > 2 ? " " : "") + argv[i];
        Case c;
        if (!parse_inputs(in.c_str(), c)) { fprintf(stderr, "does not parse: %s\n", in.c_str()); return 2; }
        walk_steps(c, plan_of(c), [&](int layer, uint32_t g, uint32_t, uint64_t, bool, const BuildStep& s) { puts(fmt_step(layer, g, s).c_str()); return true; });
        return 0;
    }
    if (mode != "check" || argc < 3) { fprintf(stderr, "usage: build_plan check TABLE | print [full] | cases [full] | steps CASE\n"); return 2; }
    FILE* fp = fopen(argv[2], "r");
    if (!fp) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    int bad = 0, lines = 0;
    std::set<std::string> seen;
    char line[1024];
    while (fgets(line, sizeof(line), fp)) {
        line[strcspn(line, "\n")] = 0;
        if (!line[0] || line[0] == '#') continue;
        lines++;
        Case c;
        if (!parse_inputs(line, c)) { printf("line %d does not parse: %s\n", lines, line); bad++; continue; }
        const std::string got = fmt_line(c, &seen);
        if (got != line) {
            if (bad < 20) printf("line %d differs\n  table: %s\n  plan:  %s\n", lines, line, got.c_str());
            bad++;
            continue;
        }
        // what the table has to hold (the line agrees with the plan, so the plan's fields are the table's)
        const BuildPlan p = plan_of(c);
        if (p.error != BuildPlanError::None) { seen.insert(std::string("error=") + build_error_name(p.error)); continue; }
        seen.insert(p.pipe ? "pipe=1" : "pipe=0");
        if (p.pipe && !p.two_a && c.tie_spill) seen.insert("one_descent_stream_by_tie_spill");
        if (p.pipe && !p.two_a && p.stream_mode == 0) seen.insert("one_descent_stream_by_knob");
        if (p.fc == 4) seen.insert("fc=4");
        if (p.smem_update > p.tile_budget || p.smem_select > p.tile_budget) seen.insert("tile_fell_back_to_64k");
        seen.insert(p.a_regs256 ? "a_regs256=1" : "a_regs256=0");
        if (!p.tab16 && !p.ext && c.knob == "default" && c.n == 40000000u) seen.insert("ids_by_n");
        if (!p.tab16 && c.knob.find("tab_ids=1") != std::string::npos) seen.insert("ids_by_knob");
    }
    fclose(fp);
    std::vector<std::string> must = {"pipe=0", "pipe=1", "one_descent_stream_by_tie_spill", "one_descent_stream_by_knob", "fc=4", "tile_fell_back_to_64k",
                                     "a_regs256=0", "a_regs256=1", "ids_by_n", "ids_by_knob", "first_of_layer_lag1",
                                     "error=extend_lds"};   // (the other three errors: see the table's header)
    for (int d = 0; d < (int)BuildDescent::kCount; d++) must.push_back(std::string("descent=") + descent_name((BuildDescent)d));
    for (const std::string& m : must)
        if (!seen.count(m)) { printf("the table holds no %s line\n", m.c_str()); bad++; }
    size_t n_full = 0;
    full_cases([&](const Case& c) {
        n_full++;
        if (const char* what = broken_property(c)) {
            if (bad < 20) printf("%s: %s\n", what, fmt_line(c).c_str());
            bad++;
        }
    });
    if (bad) { printf("%d failures (%d table lines, %zu cases)\n", bad, lines, n_full); return 1; }
    printf("build_plan ok: %d table lines, %zu cases\n", lines, n_full);
    return 0;
}
