// plan_search alone (instant-distance_amd/csrc/idist_search_plan.hpp): which walk, visited set, LDS and residency a search launch gets,
// as a pure function of plain values — on the CPU, no device.  Compiled and run by tests/test_search_plan.py.
//   search_plan check TABLE   every line of tests/golden/search_plan.txt (facts and knobs -> the plan, RECORDED from launch_search as it
//                             was before the policy became this function) against plan_search, byte for byte; the table must hold every
//                             SearchWalk and an lds_short line; then the properties below over the full cross product of the lists
//   search_plan print [full]  the table's lines (full: the cross product's) as plan_search gives them: an intended policy change is
//                             the diff of this output against the committed file
//   search_plan cases [full]  the same cases, facts and knobs only (what a recorder of launch_search's own decisions reads)
// A line: `dim n ef nq tie_cap tables knob -> walk block tab_log2 ubits wcap resident smem views wants [lds_short]`.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../instant-distance_amd/csrc/idist_search_plan.hpp"

using namespace idist;

// A case, as a table line spells it: `dim n ef nq tie_cap tables knob`, at 256 CUs.  tables: which of the lazily made tables stand
// (none / identity / principal / inline, each including the ones before it); knob: `default`, or the one test knob that is set.
enum State { kNone, kIdentity, kPrincipal, kInline, kStates };
static const char* const kStateNames[] = {"none", "identity", "principal", "inline"};
static const uint32_t kCus = 256;
struct Case {
    uint32_t dim = 0, n = 0, ef = 0, nq = 0, tie_cap = (uint32_t)kTieCap;
    int state = kNone;
    std::string knob = "default";
};
static bool knobs_of(const std::string& tok, Knobs& k) {
    if (tok == "default") return true;
    char name[32];
    unsigned v;
    if (sscanf(tok.c_str(), "%31[a-z0-9_]=%u", name, &v) != 2) return false;
    const std::string nm = name;
    if (nm == "classic") k.classic = v;
    else if (nm == "vis_bitmap") k.vis_bitmap = v;
    else if (nm == "vis_onchip") k.vis_onchip = v;
    else if (nm == "tab_log2") k.tab_log2 = v;
    else if (nm == "tab_ids") k.tab_ids = v;
    else if (nm == "tab_q16") k.tab_q16 = v;
    else if (nm == "filter") k.filter = v;
    else if (nm == "basis") k.basis = (int)v;
    else if (nm == "inl") k.inl = (int)v;
    else if (nm == "filter_waves") k.filter_waves = v;
    else if (nm == "w2_ef") k.w2_ef = v;
    else if (nm == "quad_nq") k.quad_nq = v;
    else if (nm == "latency_nq") k.latency_nq = v;
    else return false;
    return true;
}
static std::string fmt_inputs(const Case& c) {
    char buf[160];
    snprintf(buf, sizeof(buf), "%u %u %u %u %u %s %s", c.dim, c.n, c.ef, c.nq, c.tie_cap, kStateNames[c.state], c.knob.c_str());
    return buf;
}
static bool parse_inputs(const char* line, Case& c) {
    char st[16], knob[48];
    if (sscanf(line, "%u %u %u %u %u %15s %47s", &c.dim, &c.n, &c.ef, &c.nq, &c.tie_cap, st, knob) != 7) return false;
    c.knob = knob;
    for (c.state = 0; c.state < kStates && strcmp(st, kStateNames[c.state]); c.state++) {}
    Knobs k;
    return c.state < kStates && knobs_of(c.knob, k);
}
static SearchFacts facts_of(const Case& c) {
    SearchFacts f;
    f.n = c.n;
    f.L = make_layout(c.dim);
    f.n_cu = (int)kCus;
    f.template_geometry = has_template_geometry(f.L);
    f.filter_applies = filter_applies(f.n, f.L);
    f.ef = c.ef;
    f.nq = c.nq;
    f.tie_cap = c.tie_cap;
    f.dirty_words = vis_geometry(c.n).dirty_words;
    f.filter_ready = c.state >= kIdentity;
    f.principal_table = c.state >= kPrincipal;
    f.filt_format = c.state >= kPrincipal ? kFilterFormatPrincipal : (c.state == kIdentity ? kFilterFormatIdentity : kFilterFormatNone);
    f.inline_ready = c.state == kInline;
    return f;
}
static SearchPlan plan_of(const Case& c) {
    Knobs k;
    knobs_of(c.knob, k);
    return plan_search(facts_of(c), k);
}
// the plan: `walk block tab_log2 ubits wcap resident smem views wants [lds_short]`
static std::string fmt_plan(const SearchPlan& p) {
    static const char* const views[] = {"none", "identity", "principal"};
    char buf[200];
    snprintf(buf, sizeof(buf), "%s %u %u %u %u %u %zu %s%s %s%s", walk_name(p.walk), p.block, p.tab_log2, p.ubits, p.wcap, p.resident, p.smem,
             views[(int)p.filter], p.inl ? "+inl" : "", p.wants_filter ? "filter" : "-", p.wants_inline ? "+inline" : "");
    return std::string(buf) + (p.lds_short ? " lds_short" : "");
}
static const char* const kHeader = "# dim n ef nq tie_cap tables knob -> walk block tab_log2 ubits wcap resident smem views wants [lds_short]";
static std::string fmt_line(const Case& c) { return fmt_inputs(c) + " -> " + fmt_plan(plan_of(c)); }

// ---- the lists (the issue's)
static const uint32_t kDims[] = {64, 100, 128, 200, 300, 384, 512, 768, 1024, 1536};
static const uint32_t kNs[] = {1000u, 100000u, 1000000u, 10000000u, 40000000u};   // the last: beyond the quotient form's reach
static const uint32_t kEfs[] = {1, 100, 200, 400, 512, 800, 1536, 0};             // 0: ef_big(dim)
static const uint32_t kNqs[] = {1, 512, 513, 1024, 1025, 10000};
static const uint32_t kTieRaised = 512;
// an ef_search whose W alone leaves no room in 64 KiB next to the query tile: wcap * 8 + stride * 4 > 64 KiB
static uint32_t ef_big(uint32_t dim) { return 8192u - make_layout(dim).stride / 2u; }

// the default knobs, then each test knob alone
static const char* const kKnobSets[] = {"default", "classic=1", "vis_bitmap=1", "vis_onchip=1", "tab_log2=10", "tab_log2=6", "tab_ids=1", "tab_q16=1",
                                        "filter=0", "basis=1", "basis=2", "inl=0", "inl=1", "filter_waves=3", "w2_ef=200", "quad_nq=0", "latency_nq=0"};
static Case make_case(uint32_t dim, uint32_t n, uint32_t ef, uint32_t nq, int st, const char* knob = "default", uint32_t tie_cap = (uint32_t)kTieCap) {
    Case c;
    c.dim = dim; c.n = n; c.ef = ef ? ef : ef_big(dim); c.nq = nq; c.tie_cap = tie_cap; c.state = st; c.knob = knob;
    return c;
}
template <class F> static void full_cases(F emit) {
    for (uint32_t dim : kDims) for (uint32_t n : kNs) for (uint32_t ef : kEfs) for (uint32_t nq : kNqs)
        for (int st = 0; st < kStates; st++) for (const char* k : kKnobSets) for (uint32_t tie : {(uint32_t)kTieCap, kTieRaised})
            emit(make_case(dim, n, ef, nq, st, k, tie));
}
// The committed table: a selection of the cross product (every line of it is one of full_cases').
template <class F> static void table_cases(F emit_raw) {
    std::set<std::string> seen;
    auto emit = [&](const Case& c) { if (seen.insert(fmt_inputs(c)).second) emit_raw(c); };
    // every geometry, small / large / beyond the quotient form: a wide batch at a short and a long walk without and with the tables, one query
    for (uint32_t dim : kDims) for (uint32_t n : {1000u, 1000000u, 40000000u}) {
        for (uint32_t ef : {100u, 800u}) for (int st : {kNone, kInline}) emit(make_case(dim, n, ef, 10000, st));
        emit(make_case(dim, n, 100, 1, kNone));
    }
    // the geometries with kernels of their own and a long runtime one: every ef_search, every table state
    for (uint32_t dim : {128u, 300u, 768u, 1024u}) {
        for (uint32_t ef : kEfs) for (int st = 0; st < kStates; st++) emit(make_case(dim, 1000000, ef, 10000, st));
        for (uint32_t n : {100000u, 10000000u}) for (uint32_t ef : {100u, 400u}) emit(make_case(dim, n, ef, 10000, kInline));
    }
    // the batch widths around the four-wave and latency thresholds
    for (uint32_t dim : {128u, 768u}) for (uint32_t n : {1000u, 1000000u}) for (uint32_t nq : kNqs) emit(make_case(dim, n, 100, nq, kNone));
    // each test knob alone
    for (const char* k : kKnobSets)
        for (uint32_t dim : {128u, 300u, 768u}) for (uint32_t ef : {100u, 800u}) emit(make_case(dim, 1000000, ef, 10000, kInline, k));
    for (const char* k : {"classic=1", "vis_bitmap=1", "filter=0", "quad_nq=0", "latency_nq=0"})
        for (uint32_t n : {1000u, 1000000u}) for (uint32_t nq : {1u, 1024u, 10000u}) emit(make_case(128, n, 100, nq, kNone, k));
    // a raised tie capacity
    for (uint32_t dim : {128u, 300u, 768u}) for (uint32_t ef : {100u, 1536u}) emit(make_case(dim, 1000000, ef, 10000, kInline, "default", kTieRaised));
}

// ---- properties of every plan
static bool geo_thin_search(const Layout& L) {
#define THIN_OF(NB_, RS_, TAIL_) return GeoKernels<NB_>::thin_search
    IDIST_DISPATCH(L, THIN_OF);
#undef THIN_OF
    return false;
}
static bool geo_fat_filtered_search(const Layout& L, bool ids) {
#define FAT_OF(NB_, RS_, TAIL_) return ids ? GeoKernels<NB_>::fat_filtered_search_ids : GeoKernels<NB_>::fat_filtered_search
    IDIST_DISPATCH(L, FAT_OF);
#undef FAT_OF
    return false;
}
static const char* broken_property(const Case& c) {
    const SearchFacts f = facts_of(c);
    const SearchPlan p = plan_of(c), again = plan_of(c);
    if (fmt_plan(p) != fmt_plan(again)) return "planning twice from the same facts gives two plans";
    if (p.lds_short != (p.smem > 64 * 1024)) return "smem > 64 KiB without lds_short (or the reverse)";
    if (plan_q16(p.walk) && !q16_applies(p.tab_log2, p.ubits)) return "a quotient-form walk where the quotient form does not apply";
    if (plan_thin(p.walk) && !geo_thin_search(f.L)) return "a thin walk for a geometry without a thin search kernel";
    if (plan_fat_filtered(p.walk) && !geo_fat_filtered_search(f.L, p.walk == SearchWalk::FatFilteredIds)) return "a fat filtered walk for a geometry without that kernel";
    if (p.resident < kCus * 2u) return "fewer than two resident walks per CU";
    return nullptr;
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
    if (mode != "check" || argc < 3) { fprintf(stderr, "usage: search_plan check TABLE | print [full] | cases [full]\n"); return 2; }
    FILE* fp = fopen(argv[2], "r");
    if (!fp) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    int bad = 0, lines = 0;
    bool lds_short = false;
    std::set<std::string> walks;
    char line[1024];
    while (fgets(line, sizeof(line), fp)) {
        line[strcspn(line, "\n")] = 0;
        if (!line[0] || line[0] == '#') continue;
        lines++;
        Case c;
        if (!parse_inputs(line, c)) { printf("line %d does not parse: %s\n", lines, line); bad++; continue; }
        const std::string got = fmt_line(c);
        if (got != line) {
            if (bad < 20) printf("line %d differs\n  table: %s\n  plan:  %s\n", lines, line, got.c_str());
            bad++;
        }
        const char* w = strstr(line, " -> ");
        if (w) walks.insert(std::string(w + 4, strcspn(w + 4, " ")));
        if (strstr(line, " lds_short")) lds_short = true;
    }
    fclose(fp);
    for (int w = 0; w < (int)SearchWalk::kCount; w++)
        if (!walks.count(walk_name((SearchWalk)w))) { printf("the table holds no %s line\n", walk_name((SearchWalk)w)); bad++; }
    if (!lds_short) { printf("the table holds no lds_short line\n"); bad++; }
    size_t n_full = 0;
    full_cases([&](const Case& c) {
        n_full++;
        if (const char* what = broken_property(c)) {
            if (bad < 20) printf("%s: %s\n", what, fmt_line(c).c_str());
            bad++;
        }
    });
    if (bad) { printf("%d failures (%d table lines, %zu cases)\n", bad, lines, n_full); return 1; }
    printf("search_plan ok: %d table lines, %zu cases\n", lines, n_full);
    return 0;
}
