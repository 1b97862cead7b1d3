// idist_capi.hip — C ABI (include/idist.h) over the gfx950 kernels.
// Host side only orchestrates: allocation, layout conversion, launch schedule
// of the build (Hnsw::new, core/lib.rs:209-345) and of the batched search.
#include "../../include/idist.h"
#include "idist_kernels.hpp"
#include "idist_search_plan.hpp"
#include "idist_build_plan.hpp"
#include "idist_mfma.hpp"
#include "idist_combine.hpp"
#include "idist_merge.hpp"
#include "idist_normalize.hpp"
#include "idist_dot.hpp"
#include "idist_allowed.hpp"
#include "idist_range.hpp"
#include "idist_range_allowed.hpp"
#include "idist_range_merge.hpp"
#include "idist_attr.hpp"
#include "idist_grouped.hpp"
#include "idist_basis.hpp"

#ifndef IDIST_EMU
#include <hip/hip_runtime.h>
#define IDIST_LAUNCH(kfn, grid, block, smem, stream, ...) kfn<<<(grid), (block), (smem), (stream)>>>(__VA_ARGS__)
#else
#define IDIST_LAUNCH(kfn, grid, block, smem, stream, ...) \
    ::emu::launch((grid), (block), (smem), [=]() { kfn(__VA_ARGS__); })
#endif

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <time.h>
#include <vector>

using namespace idist;
static_assert(kRangeCosine == IDIST_METRIC_COSINE && kRangeDot == IDIST_METRIC_DOT && kRungNone == IDIST_RUNG_NONE && kRungExact == IDIST_RUNG_EXACT,
              "idist_range.hpp / idist_allowed.hpp restate constants of include/idist.h");
static_assert(kFilterFormatNone == IDIST_FILTER_FORMAT_NONE && kFilterFormatIdentity == IDIST_FILTER_FORMAT_IDENTITY && kFilterFormatPrincipal == IDIST_FILTER_FORMAT_PRINCIPAL,
              "idist_search_plan.hpp restates constants of include/idist.h");

// (The HIP runtime multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues — default 4, read once when the
// runtime starts.  One `Search` per host thread = one stream per thread: a host that runs more than four of them sets
// GPU_MAX_HW_QUEUES itself before its first HIP call; this library does not touch the environment.)

namespace {

// Environment knobs.  The product library (libidist.so) reads three — IDIST_COMBINE, IDIST_SYNC, IDIST_KERNEL_EVENTS: host-side
// behaviour an integrator may want to switch.  Every other IDIST_* knob exists for tests and A/B measurements and is compiled
// into the test build (libidist_variants.so, -DIDIST_VARIANTS), the measurement build (-DIDIST_PROBE) and the CPU emulator only:
// in the product test_env() is a constant nullptr, so the branches behind it fold away and no environment variable can change
// which kernels run or which graph is built.
#if defined(IDIST_VARIANTS) || defined(IDIST_PROBE) || defined(IDIST_EMU)
inline const char* test_env(const char* name) { return getenv(name); }
inline void warn_ignored_knobs() {}
#else
constexpr const char* test_env(const char*) { return nullptr; }
// The product ignores every other IDIST_* variable: say so once (a script written against the test build would otherwise measure
// the default behaviour without a hint).  The names are not known here — anything with the prefix that is not one of the three.
extern "C" char** environ;
inline void warn_ignored_knobs() {
    static std::once_flag once;
    std::call_once(once, [] {
        for (char** e = environ; e && *e; e++) {
            if (strncmp(*e, "IDIST_", 6) != 0) continue;
            const char* eq = strchr(*e, '=');
            const std::string name(*e, eq ? (size_t)(eq - *e) : strlen(*e));
            if (name == "IDIST_COMBINE" || name == "IDIST_SYNC" || name == "IDIST_KERNEL_EVENTS") continue;
            fprintf(stderr, "libidist: %s is ignored by the product library (test knobs exist in libidist_variants.so only)\n", name.c_str());
        }
    });
}
#endif

// The CU count the search side and the helper kernels size their grids by: the device's, or IDIST_CUS=<1..1024> (test knob: a small
// count makes small batches run the grid-stride loops' later trips, a large one the many short segments of a full chip; the results
// must not depend on it).  It reaches everything sized by idist_index::n_cu / idist_search_ctx::n_cu: the searches and their
// helper kernels, and also the row passes of load_points (normalise, augment), the filter tables' kernels (filter_rows_principal,
// filter_inline), bruteforce with its rerank and row-norm kernels, and the stand-alone device entry points.  Every one of these
// launches strides over its work or pulls it from a queue, and none waits for another workgroup, so any count is a legal geometry.
// plan_build alone keeps the device's count (idist_index::n_cu_build): the insertion schedule is not this knob's business.
inline int launch_cus(int device_cus) {
    if (const char* e = test_env("IDIST_CUS")) {
        const int v = atoi(e);
        if (v >= 1 && v <= 1024) return v;
    }
    return device_cus;
}

char g_err_anchor;                                      // (its address identifies this loaded library, see fresh_uid)
thread_local std::string g_err;
// The identity of an index or a partitioned index, never reused.  uids are unique across the libraries of one process too
// (libidist.so and the test build libidist_variants.so share handles in tests/): the counter starts at a value derived from where
// THIS library was mapped
uint64_t fresh_uid() {
    static std::atomic<uint64_t> next_uid{(((uint64_t)(uintptr_t)&g_err_anchor >> 12) << 28) | 1u};
    return next_uid.fetch_add(1);
}
thread_local struct idist_progress* g_watch = nullptr;   // armed by idist_progress_watch_next_build

inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield" ::: "memory");
#else
    std::this_thread::yield();
#endif
}

idist_status fail(idist_status st, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return st;
}

#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return fail(IDIST_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                        __LINE__);                                                                     \
    } while (0)

#define CHK(expr)                        \
    do {                                 \
        idist_status _s = (expr);        \
        if (_s != IDIST_OK) return _s;   \
    } while (0)

// Device scratch of a one-shot entry point: every buffer it handed out is freed when the function returns, whichever way it returns.
struct Scratch {
    std::vector<void*> owned;
    Scratch() = default;
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() { for (void* q : owned) hipFree(q); }
    template <typename T> idist_status alloc(T** p, size_t count) {
        owned.push_back(nullptr);
        HIPCHK(hipMalloc(&owned.back(), count * sizeof(T)));
        *p = (T*)owned.back();
        return IDIST_OK;
    }
};

// Grow-only device staging that frees itself: what a search context or a partitioned index keeps between calls.  Reads as the T* it
// holds; T = void for the few buffers that are read as two types (as<U>()).  Movable, so that it can live in a std::vector.
template <typename T = void> struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;                                      // bytes
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~DevBuf() { hipFree(p); }
    operator T*() const { return p; }
    template <typename U> U* as() const { return static_cast<U*>(p); }
    // p holds at least `need` BYTES afterwards, exactly `need` if it had to grow (hipFree waits for the device).  The device the
    // memory belongs on is current.  After a failed allocation p is null and cap 0, so the next call and the destructor stay safe.
    idist_status grow(size_t need) {
        if (need <= cap) return IDIST_OK;
        hipFree(p);
        p = nullptr;
        cap = 0;
        HIPCHK(hipMalloc((void**)&p, need));
        cap = need;
        return IDIST_OK;
    }
};
// `need` for the buffers that grow by doubling from `lo` bytes (0 stays 0)
inline size_t doubled_from(size_t lo, size_t need) {
    if (!need) return 0;
    while (lo < need) lo <<= 1;
    return lo;
}

idist_status check_device(int32_t device) {
    int cnt = 0;
    hipError_t e = hipGetDeviceCount(&cnt);
    if (e != hipSuccess || cnt <= 0)
        return fail(IDIST_ERR_NO_DEVICE, "no HIP device visible (%s); libidist has no CPU path",
                    e == hipSuccess ? "count = 0" : hipGetErrorString(e));
    if (device < 0 || device >= cnt) return fail(IDIST_ERR_INVALID_ARG, "device %d out of range [0,%d)", device, cnt);
    hipDeviceProp_t p;
    HIPCHK(hipGetDeviceProperties(&p, device));
    if (strncmp(p.gcnArchName, "gfx950", 6) != 0)
        return fail(IDIST_ERR_NO_DEVICE, "device %d is %s; libidist is built for gfx950 (MI355X) only", device,
                    p.gcnArchName);
    HIPCHK(hipSetDevice(device));
    return IDIST_OK;
}

idist_status validate_config(const idist_config* cfg, bool for_build) {
    if (!cfg) return fail(IDIST_ERR_INVALID_ARG, "config is null");
    if (cfg->ef_search > IDIST_MAX_EF) return fail(IDIST_ERR_INVALID_ARG, "ef_search %u > %u", cfg->ef_search, IDIST_MAX_EF);
    if (cfg->metric != IDIST_METRIC_L2SQ && cfg->metric != IDIST_METRIC_L2 && cfg->metric != IDIST_METRIC_COSINE &&
        cfg->metric != IDIST_METRIC_DOT)
        return fail(IDIST_ERR_INVALID_ARG, "unknown metric %d", cfg->metric);
    if (cfg->metric == IDIST_METRIC_DOT && !(cfg->dot_bound >= 0.0f && cfg->dot_bound < INFINITY))
        return fail(IDIST_ERR_INVALID_ARG, "dot_bound %g is not a finite number >= 0", (double)cfg->dot_bound);
    if (cfg->tie_policy != IDIST_TIES_STRICT && cfg->tie_policy != IDIST_TIES_DROP)
        return fail(IDIST_ERR_INVALID_ARG, "unknown tie_policy %d", cfg->tie_policy);
    if (cfg->tie_capacity > 4096) return fail(IDIST_ERR_INVALID_ARG, "tie_capacity %u > 4096", cfg->tie_capacity);
    if (for_build) {
        if (cfg->ef_construction == 0 || cfg->ef_construction > IDIST_MAX_EF)
            return fail(IDIST_ERR_INVALID_ARG, "ef_construction %u out of [1,%u]", cfg->ef_construction, IDIST_MAX_EF);
    }
    return IDIST_OK;
}

// IDIST_METRIC_COSINE is the squared-L2 index over normalised rows (idist_normalize.hpp): rows are normalised where they become the
// index's device copy, queries per launch, reported distances are halved — and every kernel and every policy that asks for the
// metric (IndexView.metric, the MFMA paths) sees squared L2.
inline bool is_cosine(const idist_config& cfg) { return cfg.metric == IDIST_METRIC_COSINE; }
// IDIST_METRIC_DOT is the squared-L2 index over rows with one more coordinate (idist_dot.hpp): an index keeps the caller's `dim`
// (argument checks, query strides, what it reports) and `kdim` = dim + 1 (layout, geometry, filter, every kernel launch).
inline bool is_dot(const idist_config& cfg) { return cfg.metric == IDIST_METRIC_DOT; }
inline int32_t kernel_metric(const idist_config& cfg) { return is_cosine(cfg) || is_dot(cfg) ? (int32_t)IDIST_METRIC_L2SQ : cfg.metric; }

}  // namespace

constexpr uint32_t kCombineLeaders = 8, kCombineBatch = 64;   // launches in flight per index before calls ride along; widest combined launch

// one scalar Hnsw::search call waiting to be served, alone or as part of another thread's launch (idist_combine.hpp)
struct ScalarReq {
    const float* q;
    uint32_t* pid;
    float* dist;
    uint32_t* cnt;
    uint32_t* ctr;
    idist_status st = IDIST_OK;
    std::string err;
    float kernel_ms = -1.0f;         // HIP-event duration of the launch that served this call (< 0: events are off)
    bool done = false, lead = false;
    int slot = -1;
    std::condition_variable cv;
    void fail() { st = IDIST_ERR_INTERNAL; err = "the combined launch serving this call threw (out of host memory?)"; }
};

struct idist_index {
    uint64_t uid = 0;            // never reused: a context is bound to (pointer, uid), not to the pointer alone
    mutable idist::Combiner<ScalarReq> comb{kCombineLeaders, kCombineBatch};   // scalar calls of many threads -> few launches (the index is shared, `&self`)
    // one context per leader slot for the batches a leader takes along: sized by the batches (a caller's own `Search` may be
    // backed for one query only), created on a slot's first combined launch, at most comb.max_leaders() of them
    mutable idist_search_ctx* comb_ctx[kCombineLeaders] = {nullptr};
    int32_t device = 0;
    idist_config cfg{};
    uint32_t n = 0, dim = 0;     // dim: the caller's
    uint32_t kdim = 0;           // coordinates of a stored row: dim, or dim + 1 for IDIST_METRIC_DOT — what L and every kernel see
    float dot_S = 0.0f;          // IDIST_METRIC_DOT: the bound S in use (cfg.dot_bound holds the same value once it is known)
    Layout L{};
    uint32_t n_upper = 0;
    uint32_t layer_len[IDIST_MAX_LAYERS] = {0};
    uint64_t layer_off[IDIST_MAX_LAYERS] = {0};
    size_t upper_rows = 0;
    float* d_points = nullptr;
    uint32_t* d_zero = nullptr;
    uint32_t* d_upper = nullptr;
    uint64_t* d_layer_off = nullptr;
    int n_cu = 256;          // launch_cus(): what searches and helper kernels size their grids by
    int n_cu_build = 256;    // the device's own count: plan_build's fact
    idist_build_stats stats{};
    // the walk's reject filter (FilterView, idist_device.hpp): a compact copy of the rows, made once — after a build / an import, or
    // on the first search of an index whose buffers were filled from outside (idist_index_alloc + a broadcast) — see filter_ensure
    mutable std::mutex filt_mu;
    mutable std::atomic<int> filt_state{0};    // 0 not made yet, 1 ready, 2 not available (no memory: the walks run without it)
    mutable idist::FilterView filt{};
    // ... and its second table, the 64-byte rows in a principal basis (filter_ensure: eligibility, basis, policy).  filt_format says
    // which of the two a thin wide search reads — one deterministic choice per index; everything else reads `filt`.
    mutable idist::FilterView filt_p{};        // rows == nullptr: this index has no principal table
    mutable std::atomic<int> filt_format{IDIST_FILTER_FORMAT_NONE};   // stored ONCE, when filt_p_state goes to 1 (readers: after that)
    mutable bool filt_p_turned_down = false;   // the policy chose the identity rows and no knob asked to keep the other table
    mutable std::atomic<int> filt_p_state{0};  // 0: basis, policy and principal table still to come (a build makes the identity table only:
                                               // the basis is 0.1 s of host time, which belongs to the first wide search, not to the build), 1: done
    // ... and the principal rows once more, stored with the adjacency (IndexView::inl, filter_inline_ensure): 4 KB per point
    mutable uint8_t* filt_inl = nullptr;
    mutable std::atomic<int> filt_inl_state{0};   // 0 not tried yet, 1 ready, 2 not available (above the cap, or no memory: the walks read filt_p)

    IndexView view() const {
        IndexView v;
        v.points = d_points;
        v.zero = d_zero;
        v.upper = d_upper;
        v.layer_off = d_layer_off;
        v.n = n;
        v.dim = kdim;
        v.stride = L.stride;
        v.nb = L.nb;
        v.rs = L.rs;
        v.tail = L.tail;
        v.n_upper = n_upper;
        v.metric = (uint32_t)kernel_metric(cfg);
        if (filt_state.load(std::memory_order_acquire) == 1) v.f = filt;
        return v;
    }
};

struct idist_progress {
    volatile unsigned long long* slot = nullptr;   // pinned host memory the device writes: [0] done, [1] layer + 1
    unsigned long long total = 0;
};

// The knobs (struct Knobs, idist_search_plan.hpp) as the environment sets them (see test_env above: three in the product, the rest in
// the test / measurement builds), sampled once per context or build — not per launch.
inline int filter_basis_knob(const char* e) { return e[0] == 'p' ? IDIST_FILTER_FORMAT_PRINCIPAL : (e[0] == 'i' ? IDIST_FILTER_FORMAT_IDENTITY : 0); }
inline Knobs knobs_from_env() {
    Knobs k;
    warn_ignored_knobs();
    if (const char* e = test_env("IDIST_EA")) k.ea = atoi(e);
    if (const char* e = test_env("IDIST_W2_EF")) k.w2_ef = (uint32_t)strtoul(e, nullptr, 10);
    if (const char* e = test_env("IDIST_ALLOWED_SEGMENTS")) k.allowed_segments = std::min(64u, (uint32_t)std::max(0, atoi(e)));
    if (const char* e = test_env("IDIST_RANGE_SEGMENTS")) k.range_segments = std::min(64u, (uint32_t)std::max(0, atoi(e)));
    if (const char* e = test_env("IDIST_GROUPED_STAGE")) k.grouped_stage = (uint64_t)strtoull(e, nullptr, 10);
    if (const char* e = test_env("IDIST_RANGE_SORT_CHUNK")) {
        const uint32_t c = (uint32_t)std::max(0, atoi(e));
        if (c >= 128u && c <= 4096u && (c & (c - 1u)) == 0u) k.range_sort_chunk = c;
    }
    if (const char* e = test_env("IDIST_LATENCY_NQ")) k.latency_nq = (uint32_t)strtoul(e, nullptr, 10);
    if (const char* e = test_env("IDIST_QUAD_NQ")) k.quad_nq = (uint32_t)std::min<unsigned long>(strtoul(e, nullptr, 10), 0xFFFFFFFEul);
    if (const char* e = test_env("IDIST_WALK")) k.classic = e[0] == 'c';      // (honoured by the test build only, see variants_check)
    if (const char* e = test_env("IDIST_BLOOM")) k.bloom = e[0] != '0';
    if (const char* e = test_env("IDIST_FILTER")) k.filter = e[0] != '0';
    if (const char* e = test_env("IDIST_FILTER_BASIS")) k.basis = filter_basis_knob(e);
    if (const char* e = test_env("IDIST_FILTER_INLINE")) k.inl = e[0] != '0' ? 1 : 0;
    if (const char* e = test_env("IDIST_FILTER_WAVES")) k.filter_waves = atoi(e) == 3 ? 3u : 2u;
    if (const char* e = test_env("IDIST_VISITED")) { k.vis_bitmap = e[0] == 'b'; k.vis_onchip = e[0] == 'o'; }
    if (const char* e = test_env("IDIST_NO_ZERO_COPY")) k.no_zero_copy = e[0] != '0';
    if (const char* e = test_env("IDIST_TAB_FORMAT")) { k.tab_ids = e[0] == 'i'; k.tab_q16 = e[0] == 'q'; }
    if (const char* e = getenv("IDIST_KERNEL_EVENTS")) k.events = e[0] != '0';
    if (const char* e = test_env("IDIST_TIE_SPILL")) k.tie_spill_first = e[0] == '1';
    if (const char* e = getenv("IDIST_SYNC")) k.sync_flag = e[0] != 's';
    if (const char* e = getenv("IDIST_COMBINE")) k.combine = e[0] != '0';
    if (const char* e = test_env("IDIST_TAB_LOG2")) k.tab_log2 = std::min(13u, std::max(5u, (uint32_t)atoi(e)));
    if (const char* e = test_env("IDIST_BUILD_RT")) k.build_rt = (uint32_t)atoi(e);
    if (const char* e = test_env("IDIST_BUILD_RT2")) k.build_rt2 = (uint32_t)atoi(e);
    if (const char* e = test_env("IDIST_BUILD_A2")) k.build_a2_tile = e[0] == 't';
    if (const char* e = test_env("IDIST_BUILD_PIPELINE")) k.build_pipeline = e[0] != '0';
    if (const char* e = test_env("IDIST_BUILD_A_WAVES")) k.build_a_waves = (uint32_t)std::min(8, std::max(1, atoi(e)));
    if (const char* e = test_env("IDIST_BUILD_A_REGS")) k.build_a_regs = atoi(e) == 256 ? 256 : 512;
    if (const char* e = test_env("IDIST_BUILD_QUAD")) k.build_quad = e[0] != '0';
    if (const char* e = test_env("IDIST_BUILD_GROWTH")) k.build_growth = (uint32_t)std::min(32, std::max(8, atoi(e)));
    if (const char* e = test_env("IDIST_BUILD_STREAMS")) k.build_streams = e[0] == 'o' ? 0 : (e[0] == 'a' ? 2 : 1);
    if (const char* e = test_env("IDIST_BUILD_FILTER")) k.build_filter = e[0] != '0' ? 1 : 0;
    if (test_env("IDIST_BUILD_NO_DLOG")) k.build_dlog = false;
    if (const char* e = test_env("IDIST_BUILD_CHUNK")) k.build_chunk = (uint32_t)atoi(e);
    if (test_env("IDIST_BUILD_NO_FAST")) k.build_no_fast = true;
    if (test_env("IDIST_BUILD_CHECK")) k.build_check = true;
    return k;
}

struct idist_search_ctx {
    const idist_index* idx = nullptr;
    uint64_t idx_uid = 0;          // uid of the index this context was made for
    uint32_t slots_req = 0;        // what the caller asked for (0 = as many as the batches need, up to a full chip)
    uint32_t slots = 0;            // query slots currently backed by a visited bitmap
    VisGeom vis{};
    uint32_t* d_visited = nullptr; // [slots][vis.slot_words], all-zero between launches
    uint32_t* d_next = nullptr;    // [0] queue head, [1] status, [2] completion count, [16..27] the reject filter's six 64-bit counters
    uint32_t queue_base = 0;       // value of the queue head before the next launch (it is never reset: each launch of nq queries on
                                   // g workgroups moves it by nq + g, unsigned wrap-around included)
    // narrow host-pointer batches (the reference's one query per call): query and results cross PCIe through one pinned,
    // device-mapped buffer the kernel reads and writes directly — no memcpy / memset calls around the launch
    uint8_t* h_io = nullptr;       // host address
    uint8_t* d_io = nullptr;       // the same memory as the device sees it
    size_t io_cap = 0;             // bytes of that buffer: 64 KB on first use, grown on demand up to kIoMaxBytes
    uint32_t done_seq = 0;         // completion word of the last narrow host-pointer launch (h_io + kIoStatusSlots * 4)
    double call_ns_ema = 0.0;      // how long such a call has taken lately: the host sleeps through the first half of it
    uint64_t n_flag_calls = 0;
    static constexpr size_t kIoMinBytes = 64 * 1024, kIoMaxBytes = 256 * 1024, kIoStatusSlots = 256, kIoHeadBytes = kIoStatusSlots * 4 + 64;   // ~100 queries: beyond that the staged copies are as fast (profiles/r02/probe_r02_quad_single_query_phases.jsonl)
    hipStream_t stream = nullptr;
    hipEvent_t ev0[IDIST_EVENT_RING] = {nullptr}, ev1[IDIST_EVENT_RING] = {nullptr};
    uint64_t n_launch = 0;
    // Kernel times this context reports (idist_search_ctx_kernel_times): one record per call served, in call order — its own
    // launches (slot of the event ring; resolved when asked for) and the calls that rode along in another thread's launch
    // (the leader hands the measured duration back, ScalarReq::kernel_ms)
    struct TimeRec { int32_t slot; float ms; };    // slot >= 0: own launch, event pair `slot`; slot < 0: `ms` measured elsewhere
    TimeRec recs[IDIST_EVENT_RING] = {};
    uint64_t n_rec = 0;
    int32_t device = 0;            // copies of what growing the context needs: nothing is read through `idx` after creation
    int n_cu = 256;
    Knobs knobs;
    // Every DevBuf below is staging the context owns: it only grows (byte capacities), and it frees itself when idist_search_ctx_free
    // deletes the context.  d_visited, d_next, d_tie_spill and the pinned h_io above carry state between launches and are replaced,
    // not grown; idist_search_ctx_free releases those by hand.
    // staging for the host-pointer API
    DevBuf<float> d_q, d_dist;
    DevBuf<uint32_t> d_pid, d_cnt, d_ctr;
    DevBuf<float> d_qn;            // what MetricPasses::prepare writes for a launch (launch_search): the queries the kernel reads
                                   // (cosine: normalised; DOT: with the trailing 0, [nq][kdim])
    DevBuf<float> d_sq;            // DOT indexes: s(q) per query of the launch, for the report pass
    // Staging of the ladder searches (owned and freed as above), by role.
    //  * The ladder's, shared by the restricted and the range search: the pending flags, the ascending list of the pending queries,
    //    their number and their gathered rows (al_flag, al_list, al_npend, al_pq), every query's rung and counters (al_orung, al_octr).
    //    A rung's result rows and an exact scan's segment lists use d_pid / d_dist / d_cnt / d_ctr above, the queries d_q / d_qn / d_sq.
    //  * The restricted search's: the bitmap of A or of every set (al_bits), A's ascending id list (al_ids: the single-set call), the
    //    [nq][k] result with its counts (al_o*), the merged scan of the exact step (al_m*); several sets: the set of every query, |A_s|
    //    and the start rung per set, the first rung per query (al_setof, al_size, al_start, al_first); a part of a partitioned index:
    //    the words of the caller's global bitmaps that hold its bits, as uploaded (al_raw: allowed_slice_kernel cuts al_bits out of them).
    //  * The range search's: rg_*.  What idist_search_ctx_range_fetch needs lives in buffers no other call writes: the keys in
    //    completion order, every query's count, offset and report term.  rg_list: the second pending list (a rung's copy pass still
    //    reads the list that the next rung's pending pass replaces).  The restricted range search stages its sets in the restricted
    //    search's buffers: al_bits, al_setof, |A_s| (al_size), the permitted rungs per set (al_start) and per query (al_first).
    DevBuf<uint32_t> al_flag, al_list, al_npend, al_orung, al_octr;
    DevBuf<float> al_pq;
    DevBuf<uint32_t> al_bits, al_ids, al_opid, al_ocnt, al_mpid, al_mcnt, al_setof, al_size, al_start, al_first, al_raw;
    DevBuf<> al_odist, al_mdist;   // distances: f32 to the report pass, their bits to the ranking kernels
    //  * The grouped search's, on top of the restricted search's: the groups of the [nq][k] result (gr_ogroup), the
    //    bitmaps of an exact round's chunk of pending queries and the identity that names them (gr_bits, gr_ident).
    DevBuf<uint32_t> gr_ogroup, gr_bits, gr_ident;
    // The passes a call times (ladder_timed): a pair of events each, created on first use, resolved when the call has synchronised its
    // stream.  A restricted search: a pair per select and pending pass of at most seven rungs + the exact step's two; several sets: + the
    // count pass and a pending pass in front of every launch.  A range search: three pairs per rung (select, pending, copy) + five
    // (init, the exact step's three, lims).  A grouped search: the several-sets call's, + four pairs per round of its exact step
    // (exclude, scan + merge, select, pending).  Pairs beyond kAllowedEvents are not timed.
    static constexpr uint32_t kAllowedEvents = 256;
    hipEvent_t al_ev[kAllowedEvents] = {nullptr};
    uint8_t al_ev_which[kAllowedEvents / 2] = {0};   // the slot of al_ms a pair adds to
    uint32_t al_ev_used = 0;
    // al_ms[0..2]: the last restricted search's select (+ count), pending and exact scan + merge kernels, summed over its rungs
    // (idist_search_ctx_allowed_kernel_ms); [3..5]: the last range search's select (+ init, prefix, pending, copy, lims), exact scan
    // and sort kernels (idist_search_ctx_range_kernel_ms)
    float al_ms[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    // An attribute call: the call's distinct intervals next to al_bits, which attr_bitmaps_kernel fills instead of
    // an upload; its own pair of events (created on first use) and the time they gave (idist_search_ctx_attr_bitmap_ms)
    DevBuf<uint32_t> at_lo, at_hi;
    // ... or, for a call with conditions over a table, its distinct conditions as one flat program for
    // attr_match_kernel: the clauses [n_clauses][3], then and_lims [n_and + 1], then or_lims [n_sets + 1], one upload
    DevBuf<uint32_t> at_prog;
    hipEvent_t at_ev[2] = {nullptr, nullptr};
    bool at_timed = false;
    float at_ms = 0.0f;
    DevBuf<float> rg_radius, rg_term, rg_odist;
    DevBuf<uint32_t> rg_lim, rg_cnt, rg_stepcnt, rg_exlen, rg_opid, rg_list;
    DevBuf<uint64_t> rg_off, rg_stepoff, rg_chunks, rg_keys, rg_exoff, rg_lims;
    bool rg_valid = false;         // a successful range call's results are held (until the next one, or the fetch)
    uint32_t rg_nq = 0;
    uint64_t rg_total = 0;
    int32_t rg_metric = 0;
    bool tie_overflowed = false;
    uint32_t tie_cap = 0;          // tie capacity this context escalated to (0 = the index's)
    // strict ties, last resort: one bag of n keys per slot in HBM (the reference's candidate heap is unbounded, core/lib.rs:564)
    bool tie_spill = false;        // later launches attach the bags
    bool tie_escalation_exhausted = false;
    uint64_t* d_tie_spill = nullptr;
    uint32_t spill_slots = 0, n_points = 0;
    // copies of what idist_search_ctx_status needs, so that it never reads through `idx`
    int32_t tie_policy = IDIST_TIES_STRICT;
    uint32_t base_tie_cap = kTieCap, stride = 0, last_ef = 0;
};

// A partitioned index (include/idist.h): borrowed parts + everything one caller needs to search them as one — the role of one
// `&mut Search` over all parts.  The indexes are borrowed.  The object owns a search context per non-empty part (freed by
// idist_partitioned_free), its stream and events, and every DevBuf below: staging that only grows and frees itself with the object.
struct idist_partitioned {
    uint64_t uid = 0;                        // never reused (fresh_uid): an idist_attr is bound to it, not to the address
    struct Part {
        const idist_index* idx = nullptr;
        uint64_t uid = 0;
        idist_search_ctx* ctx = nullptr;     // nullptr: empty part (nothing to search); its stream is the part's stream
        int dev_slot = 0;                    // index into `devs`
        // parts away from the merge device write here first, then one peer copy per array
        DevBuf<uint32_t> r_pid, r_cnt, r_ctr;
        DevBuf<float> r_dist;
        // range search, a part away from the merge device: its keys, offsets, counts and counters ON the merge device (peer copies on
        // the part's stream; grown with the merge device current); a part on the merge device is read where its context holds them
        DevBuf<uint64_t> m_keys, m_off;
        DevBuf<uint32_t> m_cnt, m_ctr;
    };
    struct Dev {
        int32_t device = 0;
        DevBuf<float> d_q;                   // the batch's queries, uploaded once per distinct device
        DevBuf<uint32_t> d_setof;            // restricted search: the set of every query, uploaded once per distinct device
        DevBuf<float> d_sq;                  // range search over DOT parts: s(q) of the batch's queries (the parts' limits need the report's term)
    };
    std::vector<Part> parts;
    std::vector<Dev> devs;
    uint32_t base[kMergeMaxLists + 1] = {0};
    uint32_t dim = 0;
    int32_t metric = 0, merge_device = 0;
    float dot_S = 0.0f;                      // DOT: the bound every part holds
    DevBuf<float> d_qm, d_sq;                // DOT, on the merge device: the batch's queries and their s(q), for the report after the merge
    // on the merge device: the parts' lists [P][nq][width] and the merged result [nq][out_width]
    DevBuf<uint32_t> s_pid, s_cnt, s_ctr, o_pid, o_cnt, o_ctr;
    DevBuf<float> s_dist, o_dist;
    DevBuf<uint32_t> s_rung;                 // restricted search: the parts' rungs [P][nq]
    float al_slice_ms = 0.0f;                // ... and the host time its last call spent on the bitmaps: upload + slice, every part
                                             // (an attribute call: the parts' bitmap kernels, HIP events, summed)
    // range search, on the merge device: the merged counts, lims and the chunk sums of their prefix sum; the merged result, which no
    // other call writes and idist_partitioned_range_fetch hands out once
    DevBuf<uint32_t> rm_c, rm_opid;
    DevBuf<uint64_t> rm_lims, rm_chunks;
    DevBuf<float> rm_odist;
    bool rg_valid = false;                   // a successful range call's results are held (until the next one, or the fetch)
    uint64_t rg_total = 0;
    float rg_merge_ms = -1.0f;               // the last range call's counts, prefix and merge kernels (-1: none has run)
    hipStream_t stream = nullptr;            // the merge and the copies of its result
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
};

// n_cols u32 per point on the device, next to the rows (include/idist.h): immutable after creation.  Bound to
// the handle it was made for by that handle's uid.  An index: one slice on its device; a partitioned index: one per part, empty
// parts included (n == 0, no memory), each on its part's device.  A slice holds its points of every column, column after column:
// v [n_cols][n], so that v starts with the n values of column 0 the interval calls read.  The slices free themselves.
struct idist_attr {
    uint64_t owner_uid = 0;
    bool partitioned = false;
    uint32_t n_cols = 1;
    struct Slice {
        uint32_t n = 0;
        int32_t device = 0;
        DevBuf<uint32_t> v;
    };
    std::vector<Slice> parts;
};

namespace {

// (the third wave per SIMD of a principal walk is an A/B: instantiated where the knob exists, or where it is the default)
#if defined(IDIST_VARIANTS) || defined(IDIST_EMU) || defined(IDIST_PROBE)
constexpr bool kPrincipalWaves3 = true;
#else
constexpr bool kPrincipalWaves3 = false;
#endif
template <int NB, int RS, int TAIL, int WALK, bool ON> struct SearchLaunch {
    static bool go(uint32_t grid, uint32_t block, size_t smem, hipStream_t stream, const IndexView& view, const SearchArgs& a) {
        auto kS = search_kernel<NB, RS, TAIL, WALK>;
        IDIST_LAUNCH(kS, grid, block, smem, stream, view, a);
        return true;
    }
};
template <int NB, int RS, int TAIL, int WALK> struct SearchLaunch<NB, RS, TAIL, WALK, false> {
    static bool go(uint32_t, uint32_t, size_t, hipStream_t, const IndexView&, const SearchArgs&) { return false; }
};
template <int NB, int RS, int TAIL, bool ON> struct BoundLaunch {       // filter_bound_kernel on the principal rows
    static bool go(uint32_t grid, size_t smem, const IndexView& view, const float* q, uint32_t nq, const uint32_t* ids, uint32_t n_ids, float* out) {
        auto kD = filter_bound_kernel<NB, RS, TAIL, true>;
        IDIST_LAUNCH(kD, grid, 64, smem, (hipStream_t) nullptr, view, q, nq, ids, n_ids, out);
        return true;
    }
};
template <int NB, int RS, int TAIL> struct BoundLaunch<NB, RS, TAIL, false> {
    static bool go(uint32_t, size_t, const IndexView&, const float*, uint32_t, const uint32_t*, uint32_t, float*) { return false; }
};
template <int NB, int RS, int TAIL, int WALK, bool ON> struct DescentLaunch {
    static bool go(uint32_t grid, size_t smem, hipStream_t stream, const IndexView& view, const BuildArgs& a) {
        auto kA = build_insert_kernel<NB, RS, TAIL, WALK>;
        IDIST_LAUNCH(kA, grid, 64, smem, stream, view, a);
        return true;
    }
};
template <int NB, int RS, int TAIL, int WALK> struct DescentLaunch<NB, RS, TAIL, WALK, false> {
    static bool go(uint32_t, size_t, hipStream_t, const IndexView&, const BuildArgs&) { return false; }
};

idist_status index_alloc(uint32_t n, uint32_t dim, const idist_config* cfg, const uint32_t* layer_len,
                         uint32_t n_upper, int32_t device, idist_index** out) {
    if (!out) return fail(IDIST_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    if (dim == 0 || dim > 65536) return fail(IDIST_ERR_INVALID_ARG, "dim %u out of [1,65536]", dim);
    if (is_dot(*cfg) && dim > 65535) return fail(IDIST_ERR_INVALID_ARG, "dim %u out of [1,65535] for the inner-product metric (rows hold dim + 1 coordinates)", dim);
    if (n == 0xFFFFFFFFu) return fail(IDIST_ERR_INVALID_ARG, "n must be < u32::MAX (core/lib.rs:256)");
    if (n_upper >= IDIST_MAX_LAYERS) return fail(IDIST_ERR_INVALID_ARG, "more than %u layers", IDIST_MAX_LAYERS);
    CHK(check_device(device));
    idist_index* ix = new idist_index();
    ix->uid = fresh_uid();
    ix->device = device;
    ix->cfg = *cfg;
    ix->n = n;
    ix->dim = dim;
    ix->kdim = dim + (is_dot(*cfg) ? 1u : 0u);
    ix->dot_S = is_dot(*cfg) ? cfg->dot_bound : 0.0f;     // replication targets: the source's S; builds and imports: load_points_device
    ix->L = make_layout(ix->kdim);
    ix->n_upper = n_upper;
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, device) == hipSuccess) {
        ix->n_cu_build = p.multiProcessorCount;
        ix->n_cu = launch_cus(p.multiProcessorCount);
    }
    size_t rows = 0;
    for (uint32_t l = 0; l < n_upper; l++) {
        if (layer_len[l] > n) { delete ix; return fail(IDIST_ERR_INVALID_ARG, "layer_len[%u] = %u > n", l, layer_len[l]); }
        ix->layer_len[l] = layer_len[l];
        ix->layer_off[l] = rows;
        rows += layer_len[l];
    }
    ix->upper_rows = rows;
    auto cleanup = [&](idist_status s) { idist_index_free(ix); return s; };
    auto alloc = [&](void** p, size_t bytes) -> idist_status {
        HIPCHK(hipMalloc(p, std::max<size_t>(bytes, 256)));
        return IDIST_OK;
    };
    idist_status s;
    if ((s = alloc((void**)&ix->d_points, (size_t)n * ix->L.stride * 4)) != IDIST_OK) return cleanup(s);
    if ((s = alloc((void**)&ix->d_zero, (size_t)n * IDIST_M2 * 4)) != IDIST_OK) return cleanup(s);
    if ((s = alloc((void**)&ix->d_upper, rows * IDIST_M * 4)) != IDIST_OK) return cleanup(s);
    if ((s = alloc((void**)&ix->d_layer_off, IDIST_MAX_LAYERS * 8)) != IDIST_OK) return cleanup(s);
    if (hipMemcpy(ix->d_layer_off, ix->layer_off, IDIST_MAX_LAYERS * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(ix->d_zero, 0xFF, std::max<size_t>((size_t)n * IDIST_M2 * 4, 4)) != hipSuccess ||
        hipMemset(ix->d_upper, 0xFF, std::max<size_t>(rows * IDIST_M * 4, 4)) != hipSuccess)
        return cleanup(fail(IDIST_ERR_HIP, "index initialisation failed: %s", hipGetErrorString(hipGetLastError())));
    // callers fill these buffers from their own streams (RCCL broadcast, imports): let the fills above land first
    if (hipDeviceSynchronize() != hipSuccess)
        return cleanup(fail(IDIST_ERR_HIP, "index initialisation failed: %s", hipGetErrorString(hipGetLastError())));
    *out = ix;
    return IDIST_OK;
}

// x -> x^ for n rows of `dim` coordinates, `ld` floats apart, in the layout (nb blocks, natural remainder); natural rows: ld = dim,
// nb = 0.  out may be in.  Enqueued on `stream`.
idist_status launch_normalize(const float* in, float* out, uint32_t n, uint32_t dim, uint32_t ld, uint32_t nb, float* out_norm2,
                              int n_cu, hipStream_t stream) {
    if (n == 0) return IDIST_OK;
    const uint32_t vec = (ld % 4u) == 0u && (((uintptr_t)in | (uintptr_t)out) & 15u) == 0u ? 1u : 0u;
    const uint32_t grid = std::min<uint32_t>((n + 7u) / 8u, (uint32_t)std::max(n_cu, 1) * 32u);
    IDIST_LAUNCH(normalize_rows_kernel, grid, 64, 0, stream, in, out, n, dim, ld, nb, vec, out_norm2);
    HIPCHK(hipGetLastError());
    return IDIST_OK;
}
// the factor 0.5 on `total` reported distances of a cosine index, on `stream`
idist_status launch_scale_half(float* d, size_t total, int n_cu, hipStream_t stream) {
    if (total == 0) return IDIST_OK;
    const uint32_t vec = ((uintptr_t)d & 15u) == 0u ? 1u : 0u;
    const uint32_t grid = (uint32_t)std::min<size_t>((total / 4u + 255u) / 256u + 1u, (size_t)std::max(n_cu, 1) * 8u);
    IDIST_LAUNCH(scale_half_kernel, grid, 256, 0, stream, d, total, vec);
    HIPCHK(hipGetLastError());
    return IDIST_OK;
}

// the passes of IDIST_METRIC_DOT (idist_dot.hpp), enqueued on `stream`
// s(x) of n natural rows into d_norm2; d_aug (may be nullptr): [n][dim + 1] = (row, 0), the augmented queries
idist_status launch_dot_norms(const float* d_in, uint32_t n, uint32_t dim, float* d_norm2, float* d_aug, int n_cu, hipStream_t stream) {
    if (n == 0) return IDIST_OK;
    const uint32_t grid = std::min<uint32_t>((n + 7u) / 8u, (uint32_t)std::max(n_cu, 1) * 32u);
    IDIST_LAUNCH(dot_norms_kernel, grid, 64, 0, stream, d_in, n, dim, d_norm2, d_aug);
    HIPCHK(hipGetLastError());
    return IDIST_OK;
}
// d -> 0.5f * (d - (s_q[row] + S)) over [nq][width] reported distances
idist_status launch_dot_report(float* d, const float* d_sq, float S, uint32_t nq, uint32_t width, int n_cu, hipStream_t stream) {
    const size_t total = (size_t)nq * width;
    if (total == 0) return IDIST_OK;
    const uint32_t vec = (width % 4u) == 0u && ((uintptr_t)d & 15u) == 0u ? 1u : 0u;
    const uint32_t grid = (uint32_t)std::min<size_t>((total / 4u + 255u) / 256u + 1u, (size_t)std::max(n_cu, 1) * 8u);
    IDIST_LAUNCH(dot_report_kernel, grid, 256, 0, stream, d, d_sq, S, total, width, vec);
    HIPCHK(hipGetLastError());
    return IDIST_OK;
}

// The host side of the metrics that are reductions onto the squared-L2 index (cosine: idist_normalize.hpp, DOT: idist_dot.hpp):
// ONE pass over a launch's queries in front of the kernels, ONE over the reported distances behind them — the kernels never learn
// about the metric (kernel_metric, IndexView).  Every entry point goes through this pair; one that is handed prepared queries or
// reports later itself (SearchOpts::prepared of launch_search, the brute force's `raw`) skips the call.  L2SQ and L2 enqueue nothing.
struct MetricPasses {
    int32_t metric;
    uint32_t dim, kdim;     // coordinates of a caller's query, of the row the kernels read
    float S;                // DOT: the bound in use
    int n_cu;
    explicit MetricPasses(const idist_index* ix) : metric(ix->cfg.metric), dim(ix->dim), kdim(ix->kdim), S(ix->dot_S), n_cu(ix->n_cu) {}
    explicit MetricPasses(const idist_partitioned* p)
        : metric(p->metric), dim(p->dim), kdim(p->parts[0].idx->kdim), S(p->dot_S), n_cu(p->parts[0].idx->n_cu) {}
    bool any() const { return metric == IDIST_METRIC_COSINE || metric == IDIST_METRIC_DOT; }
    // scratch for nq queries, in floats: what prepare writes for the kernels, and s(q) for report
    size_t qk_floats(uint32_t nq) const { return any() ? (size_t)nq * kdim : 0; }
    size_t sq_floats(uint32_t nq) const { return metric == IDIST_METRIC_DOT ? nq : 0; }
    bool in_place() const { return kdim == dim; }                              // prepare may write where it reads (staging copies only)
    bool report_keeps_zero() const { return metric != IDIST_METRIC_DOT; }      // a raw 0 is reported as 0
    // d_in [nq][dim] natural queries -> *d_qk: what the kernels read ([nq][kdim]: d_in itself, or d_qk_out).  DOT: s(q) to d_sq_out;
    // either output may be null.  d_qk (may be null too) is only written on success.  Enqueued on `stream`.
    idist_status prepare(const float* d_in, float* d_qk_out, float* d_sq_out, uint32_t nq, hipStream_t stream, const float** d_qk) const {
        if (metric == IDIST_METRIC_COSINE) CHK(launch_normalize(d_in, d_qk_out, nq, dim, dim, 0u, nullptr, n_cu, stream));
        if (metric == IDIST_METRIC_DOT) CHK(launch_dot_norms(d_in, nq, dim, d_sq_out, d_qk_out, n_cu, stream));
        if (d_qk) *d_qk = any() ? d_qk_out : d_in;
        return IDIST_OK;
    }
    // prepare for a staging copy d_q the library owns: in place where the rows keep their width, else into ONE more allocation of
    // `mem` ([nq][kdim] rows followed by s(q)).  *d_sq: where report finds s(q).
    idist_status prepare_own(float* d_q, Scratch& mem, uint32_t nq, hipStream_t stream, const float** d_qk, const float** d_sq) const {
        float* out = d_q;
        if (!in_place()) CHK(mem.alloc(&out, qk_floats(nq) + sq_floats(nq)));
        float* sq = sq_floats(nq) ? out + qk_floats(nq) : nullptr;
        *d_sq = sq;
        return prepare(d_q, out, sq, nq, stream, d_qk);
    }
    // [nq][width] squared-L2 distances of the index -> what the metric reports; d_sq: what prepare wrote.  Enqueued on `stream`.
    idist_status report(float* d_dist, const float* d_sq, uint32_t nq, uint32_t width, hipStream_t stream) const {
        if (metric == IDIST_METRIC_COSINE) return launch_scale_half(d_dist, (size_t)nq * width, n_cu, stream);
        if (metric == IDIST_METRIC_DOT) return launch_dot_report(d_dist, d_sq, S, nq, width, n_cu, stream);
        return IDIST_OK;
    }
};

constexpr uint32_t kDotMaxWaves = 1024;
// The bound of step 2 of the definition for n rows whose s(x) sit in d_norm2: bound_in > 0 is checked against every finite s(x),
// 0 derives the maximum.  Synchronises the device (null stream).  d_part: kDotMaxWaves + 1 u32 of device scratch.
idist_status dot_bound_of(const float* d_norm2, uint32_t n, float bound_in, uint32_t* d_part, float* S_out) {
    if (!(bound_in >= 0.0f && bound_in < INFINITY)) return fail(IDIST_ERR_INVALID_ARG, "dot_bound %g is not a finite number >= 0", (double)bound_in);
    uint32_t mbits = 0;
    if (n) {
        const uint32_t waves = std::min<uint32_t>((n + 63u) / 64u, kDotMaxWaves);
        IDIST_LAUNCH(dot_max_bits_kernel, waves, 64, 0, (hipStream_t) nullptr, d_norm2, n, d_part);
        IDIST_LAUNCH(dot_max_bits_kernel, 1, 64, 0, (hipStream_t) nullptr, reinterpret_cast<const float*>(d_part), waves, d_part + kDotMaxWaves);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpy(&mbits, d_part + kDotMaxWaves, 4, hipMemcpyDeviceToHost));
    }
    float smax;
    memcpy(&smax, &mbits, 4);
    if (bound_in > 0.0f && smax > bound_in) {               // name a row: the first one above the bound
        std::vector<float> h(n);
        HIPCHK(hipMemcpy(h.data(), d_norm2, (size_t)n * 4, hipMemcpyDeviceToHost));
        uint32_t r = 0;
        while (r < n && !(h[r] > bound_in && h[r] < INFINITY)) r++;
        return fail(IDIST_ERR_INVALID_ARG, "dot_bound %g is below the squared norm %g of row %u", (double)bound_in, (double)(r < n ? h[r] : smax), r);
    }
    *S_out = bound_in > 0.0f ? bound_in : smax;
    return IDIST_OK;
}
// natural d_nat [n][dim] -> d_out [n][stride] rows of kdim = dim + 1 coordinates in the layout (nb, natural remainder); *S_io: the
// bound given (0 = derive) on entry, the bound in use on return.  d_norm2_out (may be nullptr): s(x) per row.  Synchronises.
idist_status dot_augment_device(const float* d_nat, float* d_out, uint32_t n, uint32_t dim, uint32_t stride, uint32_t nb, float* S_io,
                                float* d_norm2_out, int n_cu) {
    Scratch mem;
    float* d_s = d_norm2_out;
    uint32_t* d_part = nullptr;
    if (!d_s) CHK(mem.alloc(&d_s, std::max<size_t>(n, 64)));
    CHK(mem.alloc(&d_part, kDotMaxWaves + 1));
    CHK(launch_dot_norms(d_nat, n, dim, d_s, nullptr, n_cu, nullptr));
    float S = 0.0f;
    CHK(dot_bound_of(d_s, n, *S_io, d_part, &S));
    if (d_out && n) {
        const size_t total = (size_t)n * stride;
        const int grid = (int)std::min<size_t>((total + 255) / 256, 65536);
        IDIST_LAUNCH(dot_augment_rows_kernel, grid, 256, 0, (hipStream_t) nullptr, d_nat, d_out, n, dim, stride, nb, d_s, S);
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
    }
    *S_io = S;
    return IDIST_OK;
}

// natural row-major device points -> blocked rows of the index (cosine: normalised there, the caller's rows are only read; DOT:
// augmented on the way, bound checked or derived).  The ONLY place rows are normalised / augmented: replicas and broadcast targets
// copy device rows that already are x^ / x~.
idist_status load_points_device(idist_index* ix, const float* d_nat) {
    if (is_dot(ix->cfg)) {
        float S = ix->cfg.dot_bound;
        CHK(dot_augment_device(d_nat, ix->d_points, ix->n, ix->dim, ix->L.stride, ix->L.nb, &S, nullptr, ix->n_cu));
        ix->dot_S = ix->cfg.dot_bound = S;
        return IDIST_OK;
    }
    if (ix->n == 0) return IDIST_OK;
    const size_t total = (size_t)ix->n * ix->L.stride;
    const int grid = (int)std::min<size_t>((total + 255) / 256, 65536);
    IDIST_LAUNCH(permute_rows_kernel, grid, 256, 0, (hipStream_t) nullptr, d_nat, ix->d_points, ix->n, ix->dim, ix->L.stride, ix->L.nb);
    HIPCHK(hipGetLastError());
    if (is_cosine(ix->cfg))
        CHK(launch_normalize(ix->d_points, ix->d_points, ix->n, ix->dim, ix->L.stride, ix->L.nb, nullptr, ix->n_cu, nullptr));
    HIPCHK(hipDeviceSynchronize());
    return IDIST_OK;
}
idist_status load_points_host(idist_index* ix, const float* h_nat) {
    if (ix->n == 0) return IDIST_OK;
    Scratch mem;
    float* d_nat = nullptr;
    CHK(mem.alloc(&d_nat, (size_t)ix->n * ix->dim));
    HIPCHK(hipMemcpy(d_nat, h_nat, (size_t)ix->n * ix->dim * 4, hipMemcpyHostToDevice));
    return load_points_device(ix, d_nat);
}

uint32_t default_slots(uint32_t n_points, int n_cu) {
    // fill the chip (16 single-wave workgroups per CU) within a memory budget for the visited bitmaps: one bit per
    // point and slot (core/types.rs:13-59), i.e. 512 MB for 4096 slots at 1M points, 5 GB at 10M
    size_t freeb = 0, totalb = 0;
    if (hipMemGetInfo(&freeb, &totalb) != hipSuccess) freeb = (size_t)8 << 30;
    const size_t budget = std::min<size_t>(freeb / 3, (size_t)64 << 30);
    const size_t vis = (size_t)vis_geometry(n_points).slot_words * 4;
    size_t s = (size_t)n_cu * 16;
    if (vis) s = std::min(s, std::max<size_t>(budget / vis, 64));
    return (uint32_t)std::max<size_t>(s, 1);
}

thread_local uint32_t g_tie_cap_msg = kTieCap;
uint32_t tie_capacity(const idist_config& cfg) { return g_tie_cap_msg = cfg.tie_capacity ? cfg.tie_capacity : (uint32_t)kTieCap; }

// IDIST_WALK=classic names walks that only the test build holds (libidist_variants.so): say so instead of running
// something else under that name
idist_status variants_check(bool classic) {
#if defined(IDIST_PROBE) && !defined(IDIST_VARIANTS)   // (the product cannot be asked: it reads no IDIST_WALK)
    if (classic) return fail(IDIST_ERR_UNSUPPORTED, "IDIST_WALK=classic selects a test-only variant of the walk: load libidist_variants.so (make -C instant-distance_amd/csrc variants)");
#endif
    (void)classic;
    return IDIST_OK;
}

idist_status device_status_to_code(uint32_t st, int32_t tie_policy) {
    if (st & kStBadRow) return fail(IDIST_ERR_BAD_GRAPH, "device met an adjacency id >= n");
    if ((st & kStTieOverflow) && tie_policy == IDIST_TIES_STRICT)
        return fail(IDIST_ERR_TIE_OVERFLOW, "more than %d live equidistant candidates beyond ef "
                    "(raise idist_config.tie_capacity, or tie_policy = IDIST_TIES_DROP keeps the nearest ones and goes on)", (int)g_tie_cap_msg);
    if (st & kStQueue)
        return fail(IDIST_ERR_INTERNAL, "a search launch found its context's work queue where no launch of this context left it: the "
                    "launches of one context must run once each, in the order they were enqueued (no graph replay, one stream)");
    if (st & kStGuard) return fail(IDIST_ERR_INTERNAL, "device-side loop guard tripped");
    return IDIST_OK;
}

// ---- build driver: the per-layer insertion schedule of Hnsw::new, core/lib.rs:304-329 ----
bool filter_applies(const idist_index* ix);
idist_status filter_ensure(const idist_index* ix, bool with_principal = true);

// a stream / an event of a one-shot entry point: destroyed when the function returns, whichever way it returns (null: never made)
struct OwnedStream {
    hipStream_t s = nullptr;
    OwnedStream() = default;
    OwnedStream(const OwnedStream&) = delete;
    OwnedStream& operator=(const OwnedStream&) = delete;
    ~OwnedStream() { if (s) hipStreamDestroy(s); }
    idist_status create() { HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); return IDIST_OK; }
    operator hipStream_t() const { return s; }
};
struct OwnedEvent {
    hipEvent_t e = nullptr;
    OwnedEvent() = default;
    OwnedEvent(const OwnedEvent&) = delete;
    OwnedEvent& operator=(const OwnedEvent&) = delete;
    ~OwnedEvent() { if (e) hipEventDestroy(e); }
    idist_status create() { HIPCHK(hipEventCreate(&e)); return IDIST_OK; }
    operator hipEvent_t() const { return e; }
};

// The build's 64 words of counters (d_small), by who writes what.  A counter block is 8 words a step clears before its selection:
// [0] n_touched, [1..5] queue heads (A, B, n_slow, B2, A2) — [3] is n_slow.
enum : uint32_t {
    kSmallCounters = 0,         // sequential schedule: the one counter block; the descents' queue head is its word 1
    kSmallQueueA = 1,           // the descents' queue head (pipelined: descent stream 0's, cleared on its own)
    kSmallStatus = 8,           // sequential schedule: the status word every kernel ORs into
    kSmallCountersPipe = 16,    // pipelined: the update stream's counter block; odd steps with inboxes of their own take the next one (24)
    kSmallStatusPipe = 32,      // pipelined: the status word
    kSmallMismatch = 40,        // IDIST_BUILD_CHECK: rows on which the two copies of the zero layer differ
    kSmallQueueA1 = 48,         // pipelined: descent stream 1's queue head
    kSmallBlock = 8, kSmallNSlow = 3, kSmallWords = 64
};

// What one step launches on, reads and writes: run_build fills it, launch_build_step<geometry> launches from it.
struct BuildStepIo {
    uint64_t k = 0;                       // step number, 1-based
    IndexView viewA, viewS;               // the zero layer the descents read / the selection and the updates write
    BuildArgs aA, aS, af;                 // descents; selection and updates (same step-A outputs, own counters); the fast update
    hipStream_t sA = nullptr, sA2 = nullptr, s2 = nullptr;   // descents, selection, updates
    hipEvent_t evA = nullptr, evA2 = nullptr, evC = nullptr; // this parity's descents / selection done; the carry-over has read its touched list
    bool own_a2 = false;
    uint32_t* cnt = nullptr;              // this step's counter block
    uint64_t* ext_work = nullptr;
    // the carry-over of the previous step's rows into this step's copy of the zero layer
    const uint32_t* z_prev = nullptr;
    uint32_t* z_cur = nullptr;
    const uint32_t *prev_touched = nullptr, *prev_cnt = nullptr;
    uint32_t prev_start = 0, prev_count = 0;
};

template <int NB, int RS, int TAIL>
idist_status launch_build_step(const BuildStep& st, const BuildPlan& p, const BuildStepIo& io) {
    const hipStream_t sA = io.sA, sA2 = io.sA2, s2 = io.s2;
    const bool own_selection = st.select_stream == SelectStream::Selection;   // (pipelined only)
    auto kAo = build_insert_kernel<NB, RS, TAIL, kWalkFatIds>;
    auto kAo16 = build_insert_kernel<NB, RS, TAIL, kWalkFatQ16>;
    auto kAq16 = build_insert_kernel<NB, RS, TAIL, kWalkFourWaveQ16>;
    auto kAo16w2 = build_insert_kernel<NB, RS, TAIL, walk_two_per_simd(NB)>;
    auto kF = build_update_fast_kernel<NB, RS, TAIL>;
    auto kB = build_update_kernel<NB, RS, TAIL>;
    auto kP = build_update_simple_kernel<NB, RS, TAIL>;
    auto kA2 = build_select_kernel<NB, RS, TAIL>;
    auto kX = build_extend_kernel<NB, RS, TAIL>;
    auto kA2m = build_select_mfma_kernel<NB, RS, TAIL>;
    switch (st.descent) {
        case BuildDescent::Extend: IDIST_LAUNCH(kX, 1, 64, p.smem_extend, sA, io.viewA, io.aA, io.ext_work, p.ext_cap); break;
#ifdef IDIST_VARIANTS
        case BuildDescent::ClassicQ16: {
            auto kA16 = build_insert_kernel<NB, RS, TAIL, kWalkClassicOnChipQ16>;
            IDIST_LAUNCH(kA16, st.gridA, 64, p.smem, sA, io.viewA, io.aA);
            break;
        }
        case BuildDescent::ClassicIds: {
            auto kA = build_insert_kernel<NB, RS, TAIL, kWalkClassicOnChipIds>;
            IDIST_LAUNCH(kA, st.gridA, 64, p.smem, sA, io.viewA, io.aA);
            break;
        }
#else
        case BuildDescent::ClassicQ16:
        case BuildDescent::ClassicIds: return fail(IDIST_ERR_INTERNAL, "the classic descents exist in the test build only");
#endif
        case BuildDescent::FourWaveQ16: IDIST_LAUNCH(kAq16, std::min(st.B, p.slots), 256, p.smem, sA, io.viewA, io.aA); break;
        case BuildDescent::ThinFiltered:
            if (!DescentLaunch<NB, RS, TAIL, walk_thin_filter(2), GeoKernels<NB>::thin_descent>::go(st.gridA, p.smem, sA, io.viewA, io.aA))
                return fail(IDIST_ERR_INTERNAL, "no filtered descent kernel for this row geometry");
            break;
        case BuildDescent::TwoPerSimd: IDIST_LAUNCH(kAo16w2, st.gridA, 64, p.smem, sA, io.viewA, io.aA); break;
        case BuildDescent::FatQ16: IDIST_LAUNCH(kAo16, st.gridA, 64, p.smem, sA, io.viewA, io.aA); break;
        case BuildDescent::FatIds: IDIST_LAUNCH(kAo, st.gridA, 64, p.smem, sA, io.viewA, io.aA); break;
        case BuildDescent::kCount: break;
    }
    if (p.pipe) {
        HIPCHK(hipEventRecord(io.evA, sA));
        HIPCHK(hipStreamWaitEvent(sA2, io.evA, 0));
        /* this step's inbox set is the one step k - 1's carry-over reads its touched list from (evC, recorded below) */
        if (own_selection && io.k > 1) HIPCHK(hipStreamWaitEvent(sA2, io.evC, 0));
        if (!own_selection) {
            IDIST_LAUNCH(copy_rows_kernel, 1024, 64, 0, s2, io.z_prev, io.z_cur, io.prev_touched, io.prev_cnt, io.prev_start, io.prev_count);
            if (io.own_a2) HIPCHK(hipEventRecord(io.evC, s2));
        }
        HIPCHK(hipMemsetAsync(io.cnt, 0, 32, sA2));
    }
    if (p.ext) {
    } else if (p.has_heuristic) {
        if (p.a2_mfma) IDIST_LAUNCH(kA2m, st.gridA2m, 256, p.smem_select_mfma, sA2, io.viewS, io.aS);
        else IDIST_LAUNCH(kA2, st.gridA2, 64, p.smem_select, sA2, io.viewS, io.aS);
        if (p.pipe && own_selection) {
            HIPCHK(hipEventRecord(io.evA2, sA2));
            HIPCHK(hipStreamWaitEvent(s2, io.evA2, 0));
            IDIST_LAUNCH(copy_rows_kernel, 1024, 64, 0, s2, io.z_prev, io.z_cur, io.prev_touched, io.prev_cnt, io.prev_start, io.prev_count);
            HIPCHK(hipEventRecord(io.evC, s2));
        }
        IDIST_LAUNCH(kF, st.gridB, 64, p.smem_update_fast, s2, io.viewS, io.af);
        IDIST_LAUNCH(kB, st.gridS, 64, p.smem_update, s2, io.viewS, io.aS);
    } else {
        IDIST_LAUNCH(kP, st.gridB, 64, (size_t)(72 * 8 + 64 * 4), s2, io.viewS, io.aS);
    }
    return IDIST_OK;
}

idist_status run_build(idist_index* ix, idist_progress* prog, bool tie_spill) {
    const uint32_t n = ix->n;
    if (prog) { prog->total = n; prog->slot[0] = n ? 1 : 0; prog->slot[1] = 0; }   // pid 0 is in from the start
    if (n <= 1) return IDIST_OK;   // pid 0 is never inserted (core/lib.rs:279-280)
    const idist_config& cfg = ix->cfg;
    const uint32_t top = ix->n_upper;

    // ---- the facts
    const VisGeom vg = vis_geometry(n);
    const Knobs knobs = knobs_from_env();
    CHK(variants_check(knobs.classic));
    BuildFacts f;
    f.n = n;
    f.L = ix->L;
    f.n_cu = ix->n_cu_build;
    f.ef_construction = cfg.ef_construction;
    f.max_batch = cfg.max_batch;
    f.has_heuristic = cfg.has_heuristic;
    f.extend_candidates = cfg.extend_candidates;
    f.metric_l2sq = kernel_metric(cfg) == IDIST_METRIC_L2SQ;
    f.tie_cap = tie_capacity(cfg);
    f.tie_spill = tie_spill;
    f.template_geometry = has_template_geometry(ix->L);
    f.filter_applies = filter_applies(ix);
    f.dirty_words = vg.dirty_words;

    // ---- the plan
    BuildPlan p = plan_build(f, knobs);
    switch (p.error) {
        case BuildPlanError::DescentLds: return fail(IDIST_ERR_INVALID_ARG, "dim/ef_construction need more than 64 KiB of LDS per wave");
        case BuildPlanError::UpdateTileLds: return fail(IDIST_ERR_INVALID_ARG, "dim %u needs %zu B of LDS per wave in the build (> 64 KiB)", ix->dim, p.smem_update);
        case BuildPlanError::SelectTileLds: return fail(IDIST_ERR_INVALID_ARG, "dim %u / ef_construction %u need %zu B of LDS per wave in the build (> 64 KiB)", ix->dim, cfg.ef_construction, p.smem_select);
        case BuildPlanError::ExtendLds: return fail(IDIST_ERR_INVALID_ARG, "dim/ef_construction need %zu B of LDS per wave with extend_candidates (> 64 KiB)", p.smem_extend);
        default: break;
    }
    const bool pipe = p.pipe, two_a = p.two_a, own_a2 = p.own_a2;
    const uint32_t cap = p.cap;

    // ---- scratch (all of it on the null stream)
    Scratch sc;
    DevBuf<uint32_t> zero2;                // pipelined: the second copy of the zero layer (or, after the final swap, the first)
    OwnedStream s1, s2, s3, s4;            // descents, updates; narrow steps: odd steps' descents, selection
    OwnedEvent evA[2], evS[2], evA2[2], evC, e0, e1;
    uint64_t* d_ext_work = nullptr;
    uint32_t* d_vis = nullptr;
    uint64_t* d_tie_spill = nullptr;
    uint32_t *d_nbr_dist = nullptr, *d_nbr_aux = nullptr, *d_row_nsel = nullptr, *d_slow = nullptr;
    uint32_t *d_edge_pid = nullptr, *d_edge_dist = nullptr, *d_head = nullptr, *d_next = nullptr, *d_touched = nullptr;
    uint32_t* d_small = nullptr;           // kSmall*
    uint64_t *d_wbuf = nullptr, *d_dlog_log = nullptr;
    uint32_t *d_dlog_pd = nullptr, *d_wcount = nullptr;
    unsigned long long* d_stats = nullptr; // [32]
    const size_t n_edges = (size_t)cap * IDIST_M2;
    const size_t n_touch = std::min<size_t>(n_edges, n);
    if (p.ext) CHK(sc.alloc(&d_ext_work, p.ext_cap));
    const size_t vis_words = (size_t)p.slots * vg.slot_words;            // one set of visited bitmaps per descent stream
    CHK(sc.alloc(&d_vis, vis_words * (two_a ? 2 : 1)));
    HIPCHK(hipMemset(d_vis, 0, vis_words * 4 * (two_a ? 2 : 1)));
    if (tie_spill) CHK(sc.alloc(&d_tie_spill, (size_t)p.slots * n));
    CHK(sc.alloc(&d_nbr_dist, (size_t)n * IDIST_M2));
    HIPCHK(hipMemset(d_nbr_dist, 0, (size_t)n * IDIST_M2 * 4));
    CHK(sc.alloc(&d_nbr_aux, (size_t)n * IDIST_M2));
    HIPCHK(hipMemset(d_nbr_aux, 0, (size_t)n * IDIST_M2 * 4));
    CHK(sc.alloc(&d_row_nsel, (size_t)n));
    HIPCHK(hipMemset(d_row_nsel, 0, (size_t)n * 4));
    const size_t nib = own_a2 ? 2 : 1;                                   // inbox sets
    CHK(sc.alloc(&d_slow, nib * n_touch));
    const size_t np = pipe ? 2 : 1;       // step-A outputs are double-buffered in the pipelined schedule
    CHK(sc.alloc(&d_wbuf, np * cap * cfg.ef_construction));
    CHK(sc.alloc(&d_wcount, np * cap));
    const size_t dl_n = cfg.has_heuristic ? (np * cap) << p.dl_shift : 64;   // the simple splice looks nothing up
    CHK(sc.alloc(&d_dlog_log, dl_n));
    CHK(sc.alloc(&d_dlog_pd, dl_n * 2));
    if (pipe) {
        CHK(zero2.grow((size_t)n * IDIST_M2 * 4));
        HIPCHK(hipMemset(zero2, 0xFF, (size_t)n * IDIST_M2 * 4));
        CHK(s1.create());
        CHK(s2.create());
        if (two_a) CHK(s3.create());
        if (own_a2) {
            CHK(s4.create());
            for (int i = 0; i < 2; i++) CHK(evA2[i].create());
            CHK(evC.create());
        }
        for (int i = 0; i < 2; i++) { CHK(evA[i].create()); CHK(evS[i].create()); }
    }
    CHK(sc.alloc(&d_edge_pid, nib * n_edges));
    CHK(sc.alloc(&d_edge_dist, nib * n_edges));
    CHK(sc.alloc(&d_next, nib * n_edges));
    CHK(sc.alloc(&d_head, nib * (size_t)n));
    HIPCHK(hipMemset(d_head, 0xFF, nib * (size_t)n * 4));
    CHK(sc.alloc(&d_touched, nib * n_touch));
    CHK(sc.alloc(&d_small, (size_t)kSmallWords));
    HIPCHK(hipMemset(d_small, 0, kSmallWords * 4));
    CHK(sc.alloc(&d_stats, 32));
    HIPCHK(hipMemset(d_stats, 0, 256));
    CHK(e0.create());
    CHK(e1.create());
    if (p.wants_filter) CHK(filter_ensure(ix, false));      // (the descents read the identity table; basis and policy wait for the first wide search)
    resolve_build_filter(p, ix->filt_state.load(std::memory_order_acquire) == 1);
    IndexView view = ix->view();
    if (!p.filtered) view.f = FilterView{};
    uint32_t* const smallS = d_small + (pipe ? kSmallCountersPipe : kSmallCounters);   // step A2/B/B2 counters (own stream)
    uint32_t* const d_status = d_small + (pipe ? kSmallStatusPipe : kSmallStatus);
    BuildArgs a{};
    a.top = top;
    a.efc = cfg.ef_construction;
    a.wcap = p.wcap;
    a.keep_pruned = cfg.keep_pruned ? 1u : 0u;
    a.has_heuristic = cfg.has_heuristic ? 1u : 0u;
    a.use_bloom = knobs.bloom ? 1u : 0u;
    a.visited = d_vis;
    a.vis = vg;
    a.edge_pid = d_edge_pid;
    a.edge_dist = d_edge_dist;
    a.head = d_head;
    a.next = d_next;
    a.touched = d_touched;
    a.nbr_dist = d_nbr_dist;
    a.row_nsel = d_row_nsel;
    a.nbr_aux = d_nbr_aux;
    a.slow = d_slow;
    a.rt = p.rt;
    a.n_touched = smallS;
    a.queue = d_small + kSmallQueueA;
    a.n_slow = d_small + kSmallCounters + kSmallNSlow;
    a.status = d_status;
    a.dlog_log = d_dlog_log;
    a.dlog_pd = d_dlog_pd;
    a.tab_log2 = p.tab_log2;
    a.tab16 = p.tab16 ? 1u : 0u;
    a.ubits = p.ubits;
    a.dl_shift = p.dl_shift;
    a.use_dlog = p.use_dlog ? 1u : 0u;
    a.wbuf = d_wbuf;
    a.wcount = d_wcount;
    a.rt2 = p.rt2;
    a.fc = p.fc;
    a.tie_cap = f.tie_cap;
    a.tie_spill = d_tie_spill;
    a.tie_spill_cap = tie_spill ? n : 0u;
    a.chunk = p.chunk;
    a.stats = d_stats;
    uint32_t cum[IDIST_MAX_LAYERS + 1];
    cum[0] = n;
    for (uint32_t l = 1; l <= top; l++) cum[l] = ix->layer_len[l - 1];
    // the set-up above ran on the null stream, which the pipeline's non-blocking streams do not wait for
    if (pipe) HIPCHK(hipDeviceSynchronize());

    // ---- the loop (a build that is not pipelined has made no stream: every role below is the null stream)
    const hipStream_t stream = s1;
    const hipStream_t descent_streams[3] = {s1, s3, s2}, select_streams[2] = {s2, s4};   // by DescentStream / SelectStream
    uint32_t* zbuf[2] = {ix->d_zero, pipe ? zero2.p : ix->d_zero};     // copy k&1 holds the state after step k
    uint64_t n_batches = 0;
    uint32_t prev_start = 0, prev_count = 0;
    HIPCHK(hipEventRecord(e0, stream));
    for (int layer = (int)top; layer >= 0; layer--) {                    // core/lib.rs:304
        const uint32_t end = cum[layer];
        uint32_t g = (uint32_t)layer == top ? 1u : std::max(cum[layer + 1], 1u);   // ranges, :275-281
        a.layer = (uint32_t)layer;
        bool first_of_layer = true;
        while (g < end) {
            const uint64_t k = n_batches + 1;                              // step number, 1-based
            const BuildStep st = plan_build_step(p, top, (uint32_t)layer, g, end, k, first_of_layer);
            const uint32_t B = st.B;
            const int par = st.par;
            a.start = g;
            a.count = B;
            BuildStepIo io;
            io.k = k;
            io.sA = descent_streams[(int)st.descent_stream];
            io.sA2 = select_streams[(int)st.select_stream];
            io.s2 = s2;
            io.own_a2 = own_a2;
            io.ext_work = d_ext_work;
            io.viewA = io.viewS = view;
            BuildArgs& aA = io.aA;
            aA = a;
            if (pipe) {
                if (k > (uint64_t)st.lag) HIPCHK(hipStreamWaitEvent(io.sA, evS[(k - st.lag) & 1u], 0));
                io.viewA.zero = zbuf[(k - st.lag) & 1u];
                io.viewS.zero = zbuf[par];
                aA.queue = d_small + (two_a && par ? kSmallQueueA1 : kSmallQueueA);   // step A queue head, one per descent stream
                if (two_a && par) aA.visited = d_vis + vis_words;
                aA.dlog_log = d_dlog_log + (((size_t)par * cap) << p.dl_shift);
                aA.dlog_pd = d_dlog_pd + (((size_t)par * cap) << (p.dl_shift + 1u));
                aA.wbuf = d_wbuf + (size_t)par * cap * cfg.ef_construction;
                aA.wcount = d_wcount + (size_t)par * cap;
                HIPCHK(hipMemsetAsync(aA.queue, 0, 4, io.sA));
                io.evA = evA[par];
                io.evA2 = evA2[par];
                io.evC = evC;
            } else {
                HIPCHK(hipMemsetAsync(d_small, 0, 32, io.sA));            // n_touched, queue heads, n_slow
            }
            BuildArgs& aS = io.aS;
            aS = aA;                                                       // same step-A outputs, own counters
            uint32_t* const cnt = smallS + (own_a2 && par ? kSmallBlock : 0);   // this step's n_touched / queue heads / n_slow
            io.cnt = cnt;
            aS.n_touched = cnt;
            aS.queue = cnt + 1;
            aS.n_slow = cnt + kSmallNSlow;
            aS.visited = d_vis;
            if (own_a2 && par) {                                           // this step's inboxes
                aS.edge_pid = d_edge_pid + n_edges; aS.edge_dist = d_edge_dist + n_edges; aS.next = d_next + n_edges;
                aS.head = d_head + n; aS.touched = d_touched + n_touch; aS.slow = d_slow + n_touch;
            }
            // (carry-over of the previous step's rows: its touched list)
            io.prev_touched = own_a2 ? d_touched + (par ? 0 : n_touch) : a.touched;
            io.prev_cnt = own_a2 ? smallS + (par ? 0 : kSmallBlock) : smallS;
            io.prev_start = prev_start;
            io.prev_count = prev_count;
            io.z_prev = zbuf[par ^ 1];
            io.z_cur = zbuf[par];
            io.af = aS;
            io.af.efc = p.no_fast ? 0u : cfg.ef_construction;             // efc = 0 makes the fast kernel defer everything
#define LAUNCH_BUILD(NB_, RS_, TAIL_) CHK((launch_build_step<NB_, RS_, TAIL_>(st, p, io)))
            IDIST_DISPATCH(ix->L, LAUNCH_BUILD);
#undef LAUNCH_BUILD
            prev_start = g;
            prev_count = B;
            g += B;
            n_batches++;
            first_of_layer = false;
            if (prog) IDIST_LAUNCH(progress_kernel, 1, 1, 0, io.s2, prog->slot, (unsigned long long)g, (unsigned long long)layer + 1ull);
            if (pipe) HIPCHK(hipEventRecord(evS[par], s2));
            if ((n_batches & 1023u) == 0) HIPCHK(hipGetLastError());
        }
        if (layer > 0) {                                                 // UpperNode::from_zero, :323-328
            const size_t total = (size_t)end * IDIST_M;
            const int grid = (int)std::min<size_t>((total + 255) / 256, 65536);
            // pipelined: behind the layer's last step on the update stream; the event the next steps' descents wait for
            // (the last step's) is recorded again behind it, so whichever stream they run on finds the snapshot taken
            IDIST_LAUNCH(snapshot_kernel, grid, 256, 0, (hipStream_t)s2, zbuf[n_batches & 1u], ix->d_upper + ix->layer_off[layer - 1] * IDIST_M, end);
            if (pipe) HIPCHK(hipEventRecord(evS[n_batches & 1u], s2));     // (both the first and the second step of the next layer wait for this one)
        }
    }
    if (pipe) {
        if (n_batches) HIPCHK(hipStreamWaitEvent(s1, evS[n_batches & 1u], 0));
        if (knobs.build_check) {
            // self-check: carry the last step over as well; now the two copies must agree on every row, or some
            // step's carry-over missed a row
            const int par = (int)(n_batches & 1u);
            IDIST_LAUNCH(copy_rows_kernel, 1024, 64, 0, (hipStream_t)s1, zbuf[par], zbuf[par ^ 1], own_a2 && par ? d_touched + n_touch : a.touched,
                         smallS + (own_a2 && par ? kSmallBlock : 0), prev_start, prev_count);
            HIPCHK(hipMemsetAsync(d_small + kSmallMismatch, 0, 4, s1));
            IDIST_LAUNCH(count_row_mismatch_kernel, 1024, 256, 0, (hipStream_t)s1, zbuf[0], zbuf[1], n, d_small + kSmallMismatch);
            uint32_t bad = 0;
            HIPCHK(hipStreamSynchronize(s1));
            HIPCHK(hipMemcpy(&bad, d_small + kSmallMismatch, 4, hipMemcpyDeviceToHost));
            if (bad) return fail(IDIST_ERR_INTERNAL, "pipelined build: the two copies of the zero layer differ on %u rows", bad);
        }
        if (n_batches & 1u) std::swap(ix->d_zero, zero2.p);              // the final state lives in copy (last step)&1; zero2 frees the other
    }
    HIPCHK(hipEventRecord(e1, stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    uint32_t status = 0;
    unsigned long long stats[32] = {0};
    HIPCHK(hipMemcpy(&status, d_status, 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(stats, d_stats, 256, hipMemcpyDeviceToHost));
    ix->stats.n_dist = stats[0];
    ix->stats.n_exp0 = stats[1];
    ix->stats.n_expU = stats[2];
    ix->stats.n_sel_pairs = stats[3];
    ix->stats.n_heur_rows = stats[4];
    ix->stats.n_updates = stats[5];
    ix->stats.n_batches = n_batches;
    ix->stats.seconds = ms * 1e-3;
    ix->stats.n_updates_fast = stats[6];
    ix->stats.n_updates_full = stats[7];
    ix->stats.n_filter_examined = stats[16];
    ix->stats.n_filter_rejected = stats[17];
    ix->stats.filter_row_bytes = p.filtered ? filt_stride(ix->L.stride) : 0u;
    // the reference's own count exists only where every selection ran in the reference's order
    ix->stats.n_heur_ref = (p.ext || (cfg.has_heuristic && p.no_fast && !p.a2_mfma && cap == 1)) ? stats[8] : 0;
    if (prog) { prog->slot[0] = n; prog->slot[1] = 0; }
#ifdef IDIST_PROBE
    fprintf(stderr, "{\"probe\": \"step_B_lookups\", \"n\": %u, \"updates_single_new\": %llu, \"updates_general\": %llu, \"lookups\": %llu, "
            "\"misses\": %llu, \"misses_member_of_previous_step\": %llu, \"misses_member_of_this_step\": %llu, \"new_vs_new_rows\": %llu, "
            "\"n_updates\": %llu, \"n_updates_full\": %llu, \"n_sel_pairs\": %llu, \"n_heur_rows\": %llu}\n",
            n, stats[9], stats[10], stats[11], stats[12], stats[13], stats[14], stats[15], stats[5], stats[7], stats[3], stats[4]);
#endif
    ix->stats.tie_overflow = (status & kStTieOverflow) ? 1 : 0;
    return device_status_to_code(status, cfg.tie_policy);
}

#ifdef IDIST_PROBE
// measurement build: the four-wave walk's segment ticks (g_quad_probe, idist_device.hpp); reset != 0 clears them after the read
extern "C" int idist_probe_quad(unsigned long long* out24, int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out24, HIP_SYMBOL(g_quad_probe), 24 * sizeof(unsigned long long)) != hipSuccess) return -2;
    if (reset) {
        unsigned long long z[24] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_quad_probe), z, sizeof(z)) != hipSuccess) return -3;
    }
    return 0;
}
// ... and the inlined thin principal walk: its zero layer (mark i in out40[i], i < 24) and the whole query slot of the inlined
// kernels (slot mark i in out40[24 + i], i < 16: QS_* in idist_device.hpp) — the rest of g_quad_probe
extern "C" int idist_probe_thin(unsigned long long* out40, int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out40, HIP_SYMBOL(g_quad_probe), 40 * sizeof(unsigned long long), 24 * sizeof(unsigned long long)) != hipSuccess) return -2;
    if (reset) {
        unsigned long long z[40] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_quad_probe), z, sizeof(z), 24 * sizeof(unsigned long long)) != hipSuccess) return -3;
    }
    return 0;
}
#endif

idist_status build_common(const void* points, bool on_device, uint32_t n, uint32_t dim, const idist_config* cfg,
                          int32_t device, idist_index** out) {
    CHK(validate_config(cfg, true));
    if (!points && n) return fail(IDIST_ERR_INVALID_ARG, "points is null");
    uint32_t cum[IDIST_MAX_LAYERS + 1];
    uint32_t nl = 1;
    cum[0] = n;
    if (n) {
        nl = layer_sizes(n, cfg->ml, cum, IDIST_MAX_LAYERS);
        if (nl == 0) return fail(IDIST_ERR_INVALID_ARG, "ml = %g yields more than %u layers", (double)cfg->ml, IDIST_MAX_LAYERS);
    }
    idist_progress* prog = g_watch;
    g_watch = nullptr;
    idist_config c = *cfg;
    const bool spill_first = test_env("IDIST_TIE_SPILL") && test_env("IDIST_TIE_SPILL")[0] == '1';   // test knob, see Knobs
    bool tie_spill = false;
    for (;;) {
        idist_index* ix = nullptr;
        CHK(index_alloc(n, dim, &c, cum + 1, n ? nl - 1 : 0, device, &ix));
        idist_status s = on_device ? load_points_device(ix, (const float*)points) : load_points_host(ix, (const float*)points);
        if (s == IDIST_OK) s = run_build(ix, prog, tie_spill);
        if (s == IDIST_OK) { *out = ix; return IDIST_OK; }
        idist_index_free(ix);
        // strict ties: the descent's tie region was too small -> build again with a larger one (x8, at most 4096 entries of
        // LDS), and when that is not enough either, with HBM bags behind it (unbounded, like the reference's heap)
        const uint32_t cap = tie_capacity(c);
        if (s != IDIST_ERR_TIE_OVERFLOW || tie_spill) return s;
        if (cap >= 4096u || spill_first) tie_spill = true;
        else c.tie_capacity = std::min<uint32_t>(4096u, cap * 8u);
    }
}

// A context belongs to ONE index: `ctx->idx == idx` alone would accept a new index that happens to live at the
// address of a freed one (its bitmaps are sized for the old n).
idist_status check_ctx(const idist_index* idx, const idist_search_ctx* ctx) {
    if (!idx || !ctx || ctx->idx != idx || ctx->idx_uid != idx->uid)
        return fail(IDIST_ERR_INVALID_ARG, "ctx does not belong to idx");
    return IDIST_OK;
}

// Back `want` query slots with visited bitmaps (Search::default() grows its scratch on first use too,
// core/lib.rs:363).  Existing slots are all-zero between launches, so growing is allocate + clear.
idist_status ensure_slots(idist_search_ctx* ctx, uint32_t want, hipStream_t stream) {
    if (want <= ctx->slots) return IDIST_OK;
    uint32_t s = 1;
    while (s < want) s <<= 1;                                    // few distinct sizes: powers of two up to the cap ...
    if (ctx->slots) s = std::max(s, ctx->slots * 8u);            // ... and at least 8x per step: growing synchronises the device
    const uint32_t cap = ctx->slots_req ? ctx->slots_req : default_slots(ctx->n_points, ctx->n_cu);
    s = std::max(std::min(s, cap), 1u);
    if (s <= ctx->slots) return IDIST_OK;
    const size_t bytes = std::max<size_t>((size_t)s * ctx->vis.slot_words * 4, 256);
    uint32_t* fresh = nullptr;
    HIPCHK(hipDeviceSynchronize());                              // nothing may still be walking on the old bitmaps
    HIPCHK(hipMalloc((void**)&fresh, bytes));
    hipError_t e = hipMemsetAsync(fresh, 0, bytes, stream);
    if (e != hipSuccess) { hipFree(fresh); return fail(IDIST_ERR_HIP, "visited bitmaps: %s", hipGetErrorString(e)); }
    hipFree(ctx->d_visited);
    ctx->d_visited = fresh;
    ctx->slots = s;
    return IDIST_OK;
}

// a forced format that cannot be served is an error, never a quiet run on the other table
idist_status filter_basis_forced_check(const idist_index* ix, int knob) {
    if (knob == IDIST_FILTER_FORMAT_PRINCIPAL && ix->filt_state.load(std::memory_order_acquire) == 1 && ix->filt_p_turned_down)
        return fail(IDIST_ERR_INVALID_ARG, "the principal format was asked for by name, but this index's policy turned that table down and freed it before "
                                           "the knob was set (set it before the index's first wide search)");
    return IDIST_OK;
}

// Long walks and where the visited bitmaps land (round 5, measured, nothing kept): ef_search 800 at 1M points test-and-sets the HBM
// bitmaps ~36k times per query, and five fresh contexts on ONE index in one process answer the same 10k queries in 72.5 / 72.9 / 79.1 /
// 82.3 / 82.4 ms while fresh replicas of the index behind fresh contexts change nothing — the spread between fresh processes is the
// CONTEXT's allocation, not the index's (profiles/r05/probe_r05b_placement_ef800_contexts_vs_replicas_c3.jsonl).  The pattern alone
// (scripts/micro/bitmap_placement.hip) is placement-independent; beside random row gathers it shows the same discrete levels (3 %): the
// 192 MB of hot bitmap lines and the row gathers compete for the 256-MiB Infinity Cache, and how well the bitmaps stay in it depends on
// physical placement.  Choosing among four candidate allocations by timing the real kernel (round 1's cure for the byte array) found a
// fast one on one box (four of five processes at 74-76 ms) and none on the next (five of five at 82.7 ms) for ~0.2 s per context: not
// kept.  Gathering the rows with the non-temporal hint (leaving the cache to the bitmaps) costs 11-15 % at every ef_search and 30 % of
// the build (`make nt`, profiles/r05/probe_r05e_rows_nontemporal_ab_c3.jsonl): the row gathers live on Infinity-Cache hits too.
// The compact copy of the rows behind the walk's reject filter (FilterView): made once per index, here.  The lattice [lo, lo + 255
// step] comes from a sample of up to 2048 rows (filter_robust_range): mean and sigma are those of the central 98 % of the sampled
// coordinates (sigma rescaled to the whole of a Gaussian), the range is mean +- 5 sigma clipped to the sample's range + a quarter sigma.  Its choice decides how many candidates the filter can
// reject, never a result — a coordinate outside it is clamped and its error is part of the row's recorded |p - p^|.  Runs on the
// null stream and waits for it (an index is immutable once it is searched; its rows are in place).
// Geometries the search kernels have no filter tile for (no compile-time instantiation and a compact row beyond the fat tile's
// thirteen 128-B chunks; the thin tile holds five), indexes the copy finds no memory for and indexes whose lattice step lies
// outside [kFilterMinStep256, kFilterMaxStep256] simply run without it (filt_state = 2).
//
// The scale range.  The test of filter_rounds, dh = (float)I * dscale > ((st + E) up)^2, is a proof only while every float step in
// it and in the canonical chain it speaks about has a RELATIVE error of 2^-24 — `up` is made of such errors — so nothing on the
// way may be a denormal, and with step256 = s the quantities are tied to s:
//   * dscale = s^2 >= 2^-116 is normal, and I is an integer, so dh is 0 or >= dscale: normal too.  (Below s ~ 1e-19, dscale has
//     a handful of significant bits — at 2^-74 it is 12 % too large and every bound exceeded the distance — and below 3.7e-23 it is 0.)
//   * E >= fq.eq >= slack * mag >= 4.8e-7 sqrt(dim) 65536 s = 2^-5 sqrt(dim) s, so the right-hand side is >= 2^-10 dim s^2: normal.
//   * filter_stage_query's e * e terms may underflow (|e| <= s / 2, and any smaller): each loses at most 2^-150, sqrt(dim) 2^-75 in
//     |q - q^| — a 4096th of slack * mag >= sqrt(dim) 2^-63, which is twice what the f32 evaluation of e needs.
//   * the canonical chain's terms (q_k - p_k)^2 may underflow for a pair the filter rejects: its float result is then up to
//     dim 2^-150 below what `up` accounts for.  A rejected pair has |q - p| >= st up' + E (up' - 1) with up' - 1 >= 2^-11, so its
//     squared distance clears st^2 (1 + 2^-10) by E^2 2^-22 >= 2^-32 dim s^2 >= dim 2^-148: the underflow cannot bring it to st^2.
//   * upwards dscale must stay finite (inf * I would "prove" anything); dh itself may overflow to +inf — then the exact product
//     is beyond FLT_MAX and a finite right-hand side is still exceeded (idist_filter_bound_batch clamps it to report a finite bound).
// So the filter is active for 2^-58 <= step256 <= 2^60 — a spread (hi - lo) of the bulk of the coordinates between 2^-42 (2.3e-13)
// and 2^76 (7.6e22), wherever the data sits — and such data is ordinary: at the lower end typical squared distances are dim 1e-26,
// at the upper end they overflow.  Outside it every walk is the unfiltered one (tests/test_data_scale.py runs both sides).
constexpr float kFilterMinStep256 = 0x1p-58f, kFilterMaxStep256 = 0x1p60f;
// the robust range of filter_ensure (reorders `vals`)
void filter_robust_range(std::vector<float>& vals, double& lo, double& hi) {
    lo = 0.0;
    hi = 1.0;
    if (!vals.empty()) {
        const size_t cnt = vals.size(), k0 = cnt / 100, k1 = cnt - 1 - cnt / 100;
        std::nth_element(vals.begin(), vals.begin() + k0, vals.end());
        const float q01 = vals[k0];
        std::nth_element(vals.begin() + k0, vals.begin() + k1, vals.end());
        const float q99 = vals[k1];
        const auto mm = std::minmax_element(vals.begin(), vals.end());
        const double mn = *mm.first, mx = *mm.second;
        double sum = 0.0, sum2 = 0.0;
        size_t m = 0;
        for (const float v : vals)
            if (v >= q01 && v <= q99) { sum += v; sum2 += (double)v * v; m++; }
        const double mean = sum / (double)std::max<size_t>(m, 1);
        const double sd = std::sqrt(std::max(0.0, sum2 / (double)std::max<size_t>(m, 1) - mean * mean)) / 0.93;
        lo = std::max(mn - 0.25 * sd, mean - 5.0 * sd);
        hi = std::min(mx + 0.25 * sd, mean + 5.0 * sd);
    }
    if (!(hi > lo) || !((hi - lo) / 65280.0 > 1e-30)) hi = lo + 1.0;      // degenerate data: any lattice is as good
}

// ---- the principal format: a second compact table, 64 bytes per row (FilterView::basis) ----
// For data whose variance sits in a few dozen directions, 56 coordinates y = B (p - mu) in a principal basis prove "this candidate is
// farther than nearest[ef-1]" almost as often as all the coordinates in the natural basis do — at one 64-B fabric request per examined
// candidate instead of three (320 B at 300-d).  The bound is the identity format's chain with one more line in front:
//     |q - p| s  >=  |B (q - p)|  =  |B (q - mu) - B (p - mu)|  >=  |q^' - p^'| - E_q - E_p
//   * B is the f32 matrix as stored; s >= sigma_max(B) is computed from those very values in f64 (principal_basis), so the first
//     step needs nothing of B but what was measured.  mu cancels exactly: both sides subtract the same f32 values.
//   * q^', p^' are lattice points lo + step256 Q (Q = 256 u for a row) of the y the kernels EVALUATE (filter_project: f64, one fma
//     per stored position); E_q, E_p = |fl(y) - y^| + the evaluation error of y, at most sqrt(56) (stride + 2) 2^-53 s |x - mu|
//     (`slack`, with a per cent to spare) + that of the subtraction itself (filter_principal_error).  All in f64, rounded up to f32.
//   * from there on it is filter_rounds' test unchanged, dh = (float)I dscale > ((st + E) up)^2, with `up` = the identity format's
//     (the float steps of the test and the canonical chain of the f32 row, which the bound still speaks about) times s.
// The lattice's range is the robust range of the LEADING component of the sample — taken over all 56 it would clamp the components
// that carry the distance.  The same step range applies; outside it, or if anything here fails, the index simply has no principal table.
//
// Policy: one deterministic choice per index, from the sample alone (a pure function of the rows: replicas and re-imports agree).
// For each format the bytes an examined candidate costs are predicted as row_bytes + (1 - share) 4 dim: 64 sample rows act as
// queries, the threshold is the distance of their 32nd nearest sample row, the candidates are the sample rows beyond it, and `share`
// is what that format's bound (the formula above, f64 on the host) rejects.  The format with fewer predicted bytes is in force
// (the principal one only while it leaves at most twice the identity rows' survivors: see `take` below);
// a principal table the policy turns down is freed again.  Beneath it the per-walk switch-off of dist_pass_filtered stays.
bool filter_principal_eligible(const idist_index* ix) {
    // thin search walks only (compact identity row within the thin tile's five chunks), rows of at least 128 coordinates; DOT's
    // extra coordinate is left alone
    return ix->n > 0 && !is_dot(ix->cfg) && ix->kdim >= 128u && filt_stride(ix->L.stride) <= 128u * (uint32_t)kFiltRtChunks &&
           (GeoKernels<-1>::thin_search || has_template_geometry(ix->L));
}
// share of (query, candidate) sample pairs a format's bound rejects.  v: [ns][c] the rows in the format's coordinates (identity: the
// coordinates themselves; principal: y), ex [ns]: what a row's E carries beside its lattice error, st [nq]: the thresholds (L2),
// far [nq][*]: the candidates of query row qrow[i]
double filter_policy_share(const std::vector<double>& v, uint32_t ns, uint32_t c, const FilterView& f, const std::vector<double>& ex_row,
                           const std::vector<double>& ex_query, const std::vector<uint32_t>& qrow, const std::vector<double>& st,
                           const std::vector<std::vector<uint32_t>>& far) {
    const double lo = f.lo, s256 = f.step256, step = 256.0 * s256;
    std::vector<int32_t> code((size_t)ns * c);
    std::vector<double> ep(ns);
    for (uint32_t r = 0; r < ns; r++) {
        double e2 = 0.0;
        for (uint32_t k = 0; k < c; k++) {
            const double x = v[(size_t)r * c + k];
            const double u = std::nearbyint(std::min(std::max((x - lo) / step, 0.0), 255.0));
            const double e = x - (lo + u * step);
            e2 += e * e;
            code[(size_t)r * c + k] = (int32_t)u * 256;
        }
        ep[r] = std::sqrt(e2) + ex_row[r];
    }
    uint64_t pairs = 0, rejected = 0;
    std::vector<int32_t> Q(c);
    for (size_t i = 0; i < qrow.size(); i++) {
        const uint32_t r = qrow[i];
        double e2 = 0.0;
        for (uint32_t k = 0; k < c; k++) {
            const double x = v[(size_t)r * c + k];
            const double q = std::nearbyint(std::min(std::max((x - lo) / s256, 0.0), 65535.0));
            const double e = x - (lo + q * s256);
            e2 += e * e;
            Q[k] = (int32_t)q;
        }
        const double eq = std::max(std::sqrt(e2) + ex_query[r], f.basis ? 16.0 * s256 : 0.0);
        for (const uint32_t p : far[i]) {
            double I = 0.0;
            const int32_t* cp = &code[(size_t)p * c];
            for (uint32_t k = 0; k < c; k++) { const double d = (double)(Q[k] - cp[k]); I += d * d; }
            const double t = (st[i] + eq + ep[p]) * (double)f.up;
            pairs++;
            if (I * s256 * s256 > t * t) rejected++;
        }
    }
    return pairs ? (double)rejected / (double)pairs : 0.0;
}
// smp: the sample of filter_ensure, [ns][stride] blocked rows; ident: the identity table's view (made).  Leaves ix->filt_p and
// ix->filt_format set; nothing it fails at is an error of the index.
idist_status filter_principal_ensure(const idist_index* ix, const std::vector<float>& smp, uint32_t ns, const FilterView& ident) {
    ix->filt_format.store(IDIST_FILTER_FORMAT_IDENTITY, std::memory_order_relaxed);     // (published by the caller's store to filt_p_state)
    if (!filter_principal_eligible(ix)) return IDIST_OK;
    constexpr int m = idist::kBasisM;
    const uint32_t stride = ix->L.stride, d = ix->kdim, nb = ix->L.nb;
    std::vector<float> xs((size_t)ns * d);
    for (uint32_t r = 0; r < ns; r++)
        for (uint32_t e = 0; e < d; e++) xs[(size_t)r * d + e] = smp[(size_t)r * stride + blocked_pos(e, nb)];
    const idist::PrincipalBasis pb = idist::principal_basis(xs.data(), ns, d, d);
    // the sample in the basis (f64), and |x - mu|; rows with a non-finite coordinate take no part in range or policy
    std::vector<double> y((size_t)ns * m), xn(ns);
    std::vector<uint8_t> finite(ns, 1);
    std::vector<float> lead;
    std::vector<double> rho;             // share of |x - mu|^2 a finite row leaves outside the basis
    for (uint32_t r = 0; r < ns; r++) {
        double d2 = 0.0;
        for (uint32_t e = 0; e < d; e++) {
            if (!(std::fabs(xs[(size_t)r * d + e]) <= 3.0e38f)) finite[r] = 0;
            const double c = (double)xs[(size_t)r * d + e] - (double)pb.mu[e];
            d2 += c * c;
        }
        xn[r] = std::sqrt(d2);
        if (!finite[r]) continue;
        double y2 = 0.0;
        for (int i = 0; i < m; i++) {
            double acc = 0.0;
            for (uint32_t e = 0; e < d; e++) acc += (double)pb.B[(size_t)i * d + e] * ((double)xs[(size_t)r * d + e] - (double)pb.mu[e]);
            y[(size_t)r * m + i] = acc;
            y2 += acc * acc;
        }
        if (d2 > 0.0) rho.push_back(std::min(1.0, std::max(0.0, 1.0 - y2 / d2)));
        const double y0 = y[(size_t)r * m];
        if (std::fabs(y0) <= 3.0e38) lead.push_back((float)y0);
    }
    double lo = 0.0, hi = 1.0;
    filter_robust_range(lead, lo, hi);
    FilterView f{};
    f.fstride = 64u;
    f.lo = (float)lo;
    f.step256 = (float)((hi - lo) / 65280.0);
    if (!(f.step256 >= kFilterMinStep256 && f.step256 <= kFilterMaxStep256) || !(std::fabs(f.lo) <= 3.0e38f)) return IDIST_OK;
    f.qscale = 1.0f / f.step256;
    f.dscale = f.step256 * f.step256;
    f.up = std::nextafter((float)((double)ident.up * pb.s * (1.0 + 1e-6)), 2.0f * ident.up * (float)pb.s);
    // queries take the principal rows while they leave at most twice the rows' 99th percentile outside the basis (+ 0.1 %)
    double rho99 = 0.0;
    if (!rho.empty()) {
        std::sort(rho.begin(), rho.end());
        rho99 = rho[std::min(rho.size() - 1, rho.size() * 99 / 100)];
    }
    f.rho_max = (float)std::min(1.0, 2.0 * rho99 + 1e-3);
    f.slack = std::nextafter((float)(std::sqrt((double)m) * (double)(stride + 2u) * 0x1p-53 * pb.s * 1.01), 1.0f);

    // policy first (host only): a table the policy turns down is never made — unless a test asks for either format by name
    std::vector<uint32_t> rows_ok;
    for (uint32_t r = 0; r < ns; r++)
        if (finite[r]) rows_ok.push_back(r);
    std::vector<uint32_t> qrow;
    std::vector<double> st;
    std::vector<std::vector<uint32_t>> far;
    const uint32_t nq = std::min<uint32_t>(64u, (uint32_t)rows_ok.size());
    for (uint32_t i = 0; i < nq; i++) {
        const uint32_t r = rows_ok[(size_t)i * rows_ok.size() / nq];
        std::vector<std::pair<double, uint32_t>> dist;
        dist.reserve(rows_ok.size());
        for (const uint32_t p : rows_ok) {
            if (p == r) continue;
            double d2 = 0.0;
            for (uint32_t e = 0; e < d; e++) { const double c = (double)xs[(size_t)r * d + e] - (double)xs[(size_t)p * d + e]; d2 += c * c; }
            dist.emplace_back(d2, p);
        }
        if (dist.size() <= 32u) continue;
        std::sort(dist.begin(), dist.end());
        qrow.push_back(r);
        st.push_back(std::sqrt(dist[31].first));
        far.emplace_back();
        for (size_t k = 32; k < dist.size(); k++) far.back().push_back(dist[k].second);
    }
    std::vector<double> xi((size_t)ns * d, 0.0), zero(ns, 0.0), ex_qi(ns, 0.0), ex_p(ns, 0.0);
    for (uint32_t r = 0; r < ns; r++) {
        if (!finite[r]) continue;
        double mx = 0.0;
        for (uint32_t e = 0; e < d; e++) { xi[(size_t)r * d + e] = xs[(size_t)r * d + e]; mx = std::max(mx, std::fabs((double)xs[(size_t)r * d + e])); }
        ex_qi[r] = (double)ident.slack * (mx + std::fabs((double)ident.lo) + 65536.0 * (double)ident.step256);
        ex_p[r] = (double)f.slack * xn[r];
    }
    FilterView fpol = f;
    fpol.basis = ix->d_points;      // (any non-null value: filter_policy_share only asks whether the view is the principal one)
    const double share_i = filter_policy_share(xi, ns, d, ident, zero, ex_qi, qrow, st, far);
    const double share_p = filter_policy_share(y, ns, (uint32_t)m, fpol, ex_p, ex_p, qrow, st, far);
    const double bytes_i = (double)ident.fstride + (1.0 - share_i) * 4.0 * (double)d;
    const double bytes_p = 64.0 + (1.0 - share_p) * 4.0 * (double)d;
    // ... and no more than twice the identity rows' survivors (+ 1 %): a survivor costs the walk a dependent round trip for its f32 row,
    // which bytes under-price on a walk bound by round trips — by bytes alone 1M x 300 rows with a 64-d latent or a 1/k^2 spectrum take
    // the principal rows (0.85 / 0.61 rejected against 0.92 / 0.90) and search 5 % / 25 % slower than on the identity rows
    const bool take = bytes_p < bytes_i && (1.0 - share_p) <= 2.0 * (1.0 - share_i) + 0.01;
    if (!take && !test_env("IDIST_FILTER_BASIS")) { ix->filt_p_turned_down = true; return IDIST_OK; }

    // the table: B^T and mu in the rows' stored order, then one wave per row
    std::vector<float> bt((size_t)stride * 64u, 0.0f), mu(stride, 0.0f);
    for (uint32_t e = 0; e < d; e++) {
        const uint32_t pos = blocked_pos(e, nb);
        mu[pos] = pb.mu[e];
        for (int i = 0; i < m; i++) bt[(size_t)pos * 64u + (uint32_t)i] = pb.B[(size_t)i * d + e];
    }
    float *d_bt = nullptr, *d_mu = nullptr;
    uint8_t* rows = nullptr;
    auto drop = [&]() { (void)hipGetLastError(); hipFree(d_bt); hipFree(d_mu); hipFree(rows); };
    if (hipMalloc((void**)&d_bt, bt.size() * 4) != hipSuccess || hipMalloc((void**)&d_mu, mu.size() * 4) != hipSuccess ||
        hipMalloc((void**)&rows, (size_t)ix->n * 64u) != hipSuccess ||
        hipMemcpy(d_bt, bt.data(), bt.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_mu, mu.data(), mu.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        drop();
        return IDIST_OK;                                                  // no memory: the identity table serves
    }
    f.basis = d_bt;
    f.mu = d_mu;
    IndexView view = ix->view();
    view.f = f;
    const uint32_t grid = std::min<uint32_t>(ix->n, (uint32_t)ix->n_cu * 32u);
    IDIST_LAUNCH(filter_rows_principal_kernel, grid, 64, 0, nullptr, view, rows);
    if (hipDeviceSynchronize() != hipSuccess) {
        const hipError_t e = hipGetLastError();
        drop();
        return fail(IDIST_ERR_HIP, "filter_rows_principal_kernel failed: %s", hipGetErrorString(e));
    }
    f.rows = rows;
    ix->filt_p = f;
    if (take) ix->filt_format.store(IDIST_FILTER_FORMAT_PRINCIPAL, std::memory_order_relaxed);
    return IDIST_OK;
}
// The principal rows stored with the adjacency (IndexView::inl): block i = filt_p.rows[id] of the ids in zero row i.  Made at the
// first wide search of an index whose thin walks read the principal rows; 64 times the principal table, so above kFilterInlineCapBytes
// — or when the allocation fails — the index keeps none and its walks read filt_p as before: not an error.
// The cap: 1M points take 4.1 GB (the benchmark's index), the 2M an 8-GiB cap admits are where the table still leaves most of a 288-GB
// card to rows of 1.2 KB each and their graph; beyond it the gain of one round trip per expansion is not worth a memory footprint
// four times the rows' own.  (IDIST_FILTER_INLINE_CAP=<bytes>: test build.)
constexpr uint64_t kFilterInlineCapBytes = 8ull << 30;
idist_status filter_inline_ensure(const idist_index* ix) {
    if (ix->filt_inl_state.load(std::memory_order_acquire) != 0) return IDIST_OK;
    std::lock_guard<std::mutex> lk(ix->filt_mu);
    if (ix->filt_inl_state.load(std::memory_order_acquire) != 0) return IDIST_OK;
    HIPCHK(hipSetDevice(ix->device));
    uint64_t cap = kFilterInlineCapBytes;
    if (const char* e = test_env("IDIST_FILTER_INLINE_CAP")) cap = strtoull(e, nullptr, 10);
    const uint64_t bytes = (uint64_t)ix->n * idist::kInlineBlockBytes;
    uint8_t* blocks = nullptr;
    if (!ix->filt_p.rows || ix->filt_p.fstride != 64u || bytes > cap || hipMalloc((void**)&blocks, bytes) != hipSuccess) {
        (void)hipGetLastError();
        ix->filt_inl_state.store(2, std::memory_order_release);
        return IDIST_OK;
    }
    const uint32_t grid = std::min<uint32_t>(ix->n, (uint32_t)ix->n_cu * 32u);
    IDIST_LAUNCH(filter_inline_kernel, grid, 64, 0, nullptr, ix->d_zero, ix->filt_p.rows, ix->n, blocks);
    if (hipDeviceSynchronize() != hipSuccess) {
        const hipError_t e = hipGetLastError();
        hipFree(blocks);
        return fail(IDIST_ERR_HIP, "filter_inline_kernel failed: %s", hipGetErrorString(e));
    }
    ix->filt_inl = blocks;
    ix->filt_inl_state.store(1, std::memory_order_release);
    return IDIST_OK;
}
bool filter_applies(const idist_index* ix) { return idist::filter_applies(ix->n, ix->L); }
idist_status filter_ensure(const idist_index* ix, bool with_principal) {
    auto settled = [&]() {
        const int st = ix->filt_state.load(std::memory_order_acquire);
        return st == 2 || (st == 1 && (!with_principal || ix->filt_p_state.load(std::memory_order_acquire) == 1));
    };
    if (settled()) return IDIST_OK;
    std::lock_guard<std::mutex> lk(ix->filt_mu);
    if (settled()) return IDIST_OK;
    if (!filter_applies(ix)) { ix->filt_state.store(2, std::memory_order_release); return IDIST_OK; }
    HIPCHK(hipSetDevice(ix->device));
    const uint32_t stride = ix->L.stride, fs = filt_stride(stride);
    // sample: up to 2048 rows, evenly spaced
    const uint32_t ns = std::min<uint32_t>(ix->n, 2048u), every = ix->n / ns;
    std::vector<float> smp((size_t)ns * stride);
    HIPCHK(hipMemcpy2D(smp.data(), (size_t)stride * 4, ix->d_points, (size_t)every * stride * 4, (size_t)stride * 4, ns, hipMemcpyDeviceToHost));
    if (ix->filt_state.load(std::memory_order_acquire) == 1) {          // the identity table stands (a build made it): the second one now
        CHK(filter_principal_ensure(ix, smp, ns, ix->filt));
        ix->filt_p_state.store(1, std::memory_order_release);
        return IDIST_OK;
    }
    // robust range: mean and sigma of the central 98 % of the sampled coordinates (a few wild values — or heavy tails — must not
    // stretch the lattice: they are clamped, and only their own rows pay for it), sigma rescaled to the whole of a Gaussian
    std::vector<float> vals;
    vals.reserve((size_t)ns * ix->kdim);
    for (uint32_t r = 0; r < ns; r++)
        for (uint32_t pos = 0; pos < stride; pos++) {
            if (natural_pos(pos, ix->L.nb) >= ix->kdim) continue;
            const float v = smp[(size_t)r * stride + pos];
            if (std::fabs(v) <= 3.0e38f) vals.push_back(v);
        }
    double lo = 0.0, hi = 1.0;
    filter_robust_range(vals, lo, hi);
    FilterView f{};
    f.fstride = fs;
    f.lo = (float)lo;
    f.step256 = (float)((hi - lo) / 65280.0);                            // 255 steps of 256 sub-steps
    if (!(f.step256 >= kFilterMinStep256 && f.step256 <= kFilterMaxStep256)) {      // (see above: the bound would be no proof)
        ix->filt_state.store(2, std::memory_order_release);
        return IDIST_OK;
    }
    f.qscale = 1.0f / f.step256;
    f.dscale = f.step256 * f.step256;
    // every float step of the test (the conversion of I, dscale, the sums, the canonical chain of dim / 8 + 7 roundings) is covered
    f.up = 1.0f + 4.8828125e-4f + 6.0e-8f * (float)(ix->L.stride / 8u + 8u);
    f.slack = 4.8e-7f * std::sqrt((float)ix->kdim);
    uint8_t* rows = nullptr;
    if (hipMalloc((void**)&rows, (size_t)ix->n * fs) != hipSuccess) {
        (void)hipGetLastError();
        ix->filt_state.store(2, std::memory_order_release);
        return IDIST_OK;
    }
    const uint32_t grid = std::min<uint32_t>(ix->n, (uint32_t)ix->n_cu * 32u);
    IDIST_LAUNCH(filter_rows_kernel, grid, 64, 0, nullptr, ix->d_points, ix->n, ix->kdim, stride, ix->L.nb, rows, fs, f.lo, f.step256);
    if (hipDeviceSynchronize() != hipSuccess) {
        const hipError_t e = hipGetLastError();
        hipFree(rows);
        return fail(IDIST_ERR_HIP, "filter_rows_kernel failed: %s", hipGetErrorString(e));
    }
    f.rows = rows;
    ix->filt = f;
    if (with_principal) {
        if (const idist_status ps = filter_principal_ensure(ix, smp, ns, f); ps != IDIST_OK) {
            hipFree(rows);
            ix->filt = FilterView{};
            return ps;
        }
        ix->filt_p_state.store(1, std::memory_order_release);
    }
    ix->filt_state.store(1, std::memory_order_release);
    return IDIST_OK;
}

// What a caller may add to a plain launch of the index's own ef_search
struct SearchOpts {
    uint32_t* status_host = nullptr;   // pinned words the kernel writes its slots' status to (narrow host-pointer batches)
    uint32_t* grid_out = nullptr;      // the launch's grid
    uint32_t* done_host = nullptr;     // pinned completion word, written with done_seq
    uint32_t done_seq = 0;
    bool prepared = false;             // d_q already holds what the kernels read and the caller reports later (the partitioned search: after its merge)
    uint32_t ef = 0;                   // the ef_search of this launch when it is not the index's (the rungs of a restricted search: the index
                                       // is shared and never mutated)
    bool* lds_short = nullptr;         // set when the launch was refused because this ef_search does not fit a wave's LDS
};
// the state of the lazily made tables into the facts; true when one of them differs from what `f` held
bool table_facts(const idist_index* ix, SearchFacts& f) {
    const bool ready = ix->filt_state.load(std::memory_order_acquire) == 1;
    const bool table = ready && ix->filt_p_state.load(std::memory_order_acquire) == 1 && ix->filt_p.rows;   // (filt_p is written before its state)
    const int format = table ? ix->filt_format.load(std::memory_order_relaxed) : IDIST_FILTER_FORMAT_NONE;
    const bool inl = ix->filt_inl_state.load(std::memory_order_acquire) == 1;
    const bool changed = ready != f.filter_ready || table != f.principal_table || format != f.filt_format || inl != f.inline_ready;
    f.filter_ready = ready;
    f.principal_table = table;
    f.filt_format = format;
    f.inline_ready = inl;
    return changed;
}

// One search launch: the facts of this index, context and call -> the plan (plan_search, idist_search_plan.hpp: which kernel, which
// visited set, how much LDS, how many resident walks) -> the tables the plan wants -> the launch.
idist_status launch_search(const idist_index* ix, idist_search_ctx* ctx, const float* d_q, uint32_t nq,
                           uint32_t* d_pid, float* d_dist, uint32_t* d_cnt, uint32_t* d_ctr, hipStream_t stream,
                           const SearchOpts& o = SearchOpts()) {
    const uint32_t ef = o.ef ? o.ef : ix->cfg.ef_search;
    if (o.lds_short) *o.lds_short = false;
    const Knobs& knobs = ctx->knobs;
    CHK(variants_check(knobs.classic));
    // Cosine and DOT: the walk reads the queries MetricPasses::prepare wrote into buffers this context owns (the caller's are only
    // read), and the distances it wrote are reported behind it — both on the launch's stream, outside the events that time the
    // search kernel.
    const MetricPasses metric(ix);
    const bool passes = metric.any() && !o.prepared;
    if (passes) {
        CHK(ctx->d_qn.grow(doubled_from(4096, metric.qk_floats(nq) * 4)));
        CHK(ctx->d_sq.grow(doubled_from(256, metric.sq_floats(nq) * 4)));
        CHK(metric.prepare(d_q, ctx->d_qn, ctx->d_sq, nq, stream, &d_q));
    }
    // ---- facts
    SearchFacts facts;
    facts.n = ix->n;
    facts.L = ix->L;
    facts.n_cu = ix->n_cu;
    facts.template_geometry = has_template_geometry(ix->L);
    facts.filter_applies = filter_applies(ix);
    facts.ef = ef;
    facts.nq = nq;
    facts.tie_cap = std::max(tie_capacity(ix->cfg), ctx->tie_cap);
    facts.dirty_words = ctx->vis.dirty_words;
    table_facts(ix, facts);
    // ---- plan, and the tables it wants (made on first use; once they stand or are turned down the first plan is the launch's)
    SearchPlan plan = plan_search(facts, knobs);
    if (plan.wants_filter) {
        CHK(filter_ensure(ix));
        if (table_facts(ix, facts)) plan = plan_search(facts, knobs);
    }
    if (plan.wants_filter && facts.filter_ready) CHK(filter_basis_forced_check(ix, knobs.basis));
    if (plan.wants_inline) {
        CHK(filter_inline_ensure(ix));
        if (table_facts(ix, facts)) plan = plan_search(facts, knobs);
    }
    // ---- launch
    SearchArgs a{};
    a.queries = d_q;
    a.nq = nq;
    a.ef = ef;
    a.tie_cap = facts.tie_cap;
    a.wcap = plan.wcap;
    a.vis = ctx->vis;
    a.tab_log2 = plan.tab_log2;
    a.ubits = plan.ubits;
    uint32_t resident = plan.resident;
    if (ctx->tie_spill) {
        // one bag of n keys per slot (a walk can hold every point as a tie at most once); the slots that fit 1 GiB
        const uint32_t fit = (uint32_t)std::max<size_t>(1, ((size_t)1 << 30) / ((size_t)std::max(ix->n, 1u) * 8));
        resident = std::min(resident, fit);
        if (!ctx->d_tie_spill || ctx->spill_slots < std::min(nq, resident)) {
            HIPCHK(hipDeviceSynchronize());
            hipFree(ctx->d_tie_spill);
            ctx->d_tie_spill = nullptr;
            ctx->spill_slots = std::min(std::max(nq, 1u), resident);
            HIPCHK(hipMalloc((void**)&ctx->d_tie_spill, (size_t)ctx->spill_slots * std::max(ix->n, 1u) * 8));
        }
        resident = std::min(resident, ctx->spill_slots);
        a.tie_spill = ctx->d_tie_spill;
        a.tie_spill_cap = ix->n;
    }
    CHK(ensure_slots(ctx, std::min(nq, resident), stream));
    ctx->last_ef = ef;
    a.out_pid = d_pid;
    a.out_dist = d_dist;
    a.out_count = d_cnt;
    a.out_counters = d_ctr;
    a.visited = ctx->d_visited;
    a.next = ctx->d_next;
    a.status = ctx->d_next + 1;
    a.use_bloom = knobs.bloom ? 1u : 0u;
    const size_t smem = plan.smem;
    if (plan.lds_short) {
        if (o.lds_short) *o.lds_short = true;
        return fail(IDIST_ERR_INVALID_ARG, "dim/ef_search need %zu B of LDS per wave (> 64 KiB)", smem);
    }
    const uint32_t grid = std::min(std::min(nq, ctx->slots), resident);
    IndexView view = ix->view();
    if (plan.filter == PlanFilter::None) view.f = FilterView{};
    if (plan.filter == PlanFilter::Principal) { view.f2 = view.f; view.f = ix->filt_p; }       // (f2: the identity rows, for the queries the basis does not fit)
    if (plan.inl) view.inl = ix->filt_inl;
    a.queue_base = ctx->queue_base;
    a.status_host = o.status_host && grid <= idist_search_ctx::kIoStatusSlots ? o.status_host : nullptr;
    a.done_host = o.done_host;
    a.done_count = ctx->d_next + 2;
    a.filt_counts = reinterpret_cast<unsigned long long*>(ctx->d_next + 16);       // [6]: + the share of both on the principal rows, + the inlined blocks
    a.done_seq = o.done_seq;
    if (o.grid_out) *o.grid_out = grid;
    const uint32_t slot = (uint32_t)(ctx->n_launch % IDIST_EVENT_RING);
    if (knobs.events) HIPCHK(hipEventRecord(ctx->ev0[slot], stream));
// The `classic` walks (one distance round in flight, no adjacency prefetch) are selected by no policy: they exist as
// independent implementations of the same decisions for the parity tests and are compiled into the TEST build only
// (`make variants` -> libidist_variants.so, -DIDIST_VARIANTS; the CPU emulator build defines it too).
#ifdef IDIST_VARIANTS
#define IDIST_VARIANT_SEARCH_CASES(NB_, RS_, TAIL_)                                                                  \
    case SearchWalk::ClassicOnChipQ16: SEARCH_CASE(NB_, RS_, TAIL_, kWalkClassicOnChipQ16, true); break;             \
    case SearchWalk::ClassicOnChipIds: SEARCH_CASE(NB_, RS_, TAIL_, kWalkClassicOnChipIds, true); break;             \
    case SearchWalk::ClassicBitmap: SEARCH_CASE(NB_, RS_, TAIL_, kWalkClassic, true); break;
#else
#define IDIST_VARIANT_SEARCH_CASES(NB_, RS_, TAIL_)
#endif
    bool launched = true;
    // (ON_ = false: this geometry is never given that walk and has no instantiation of it — reaching it is the internal error below)
#define SEARCH_CASE(NB_, RS_, TAIL_, WALK_, ON_) launched = SearchLaunch<NB_, RS_, TAIL_, WALK_, ON_>::go(grid, plan.block, smem, stream, view, a)
#define LAUNCH_SEARCH(NB_, RS_, TAIL_)                                                                                                 \
    switch (plan.walk) {                                                                                                               \
        case SearchWalk::QuadQ16: SEARCH_CASE(NB_, RS_, TAIL_, kWalkFourWaveQ16, true); break;                                         \
        case SearchWalk::QuadIds: SEARCH_CASE(NB_, RS_, TAIL_, kWalkFourWaveIds, true); break;                                         \
        case SearchWalk::ThinPrincipal3: SEARCH_CASE(NB_, RS_, TAIL_, walk_thin_filter_principal(3), GeoKernels<NB_>::thin_search && kPrincipalWaves3); break; \
        case SearchWalk::ThinInline: SEARCH_CASE(NB_, RS_, TAIL_, walk_thin_filter_inline(2), GeoKernels<NB_>::thin_search); break;    \
        case SearchWalk::ThinPrincipal: SEARCH_CASE(NB_, RS_, TAIL_, walk_thin_filter_principal(2), GeoKernels<NB_>::thin_search); break; \
        case SearchWalk::ThinIdentity: SEARCH_CASE(NB_, RS_, TAIL_, walk_thin_filter(2), GeoKernels<NB_>::thin_search); break;         \
        case SearchWalk::TwoPerSimd: SEARCH_CASE(NB_, RS_, TAIL_, walk_two_per_simd(NB_), true); break;                                \
        case SearchWalk::FatFilteredIds: SEARCH_CASE(NB_, RS_, TAIL_, walk_with_filter(kWalkFatIds), GeoKernels<NB_>::fat_filtered_search_ids); break; \
        case SearchWalk::FatFilteredQ16: SEARCH_CASE(NB_, RS_, TAIL_, walk_with_filter(kWalkFatQ16), GeoKernels<NB_>::fat_filtered_search); break; \
        case SearchWalk::OnChipQ16: SEARCH_CASE(NB_, RS_, TAIL_, kWalkFatQ16, true); break;                                            \
        case SearchWalk::OnChipIds: SEARCH_CASE(NB_, RS_, TAIL_, kWalkFatIds, true); break;                                            \
        case SearchWalk::Latency: SEARCH_CASE(NB_, RS_, TAIL_, kWalkLatency, true); break;                                             \
        case SearchWalk::OverlapBitmap: SEARCH_CASE(NB_, RS_, TAIL_, kWalkOverlap, true); break;                                       \
        IDIST_VARIANT_SEARCH_CASES(NB_, RS_, TAIL_)                                                                                    \
        default: launched = false; break;                                                                                              \
    }
#ifdef IDIST_EA_PROBE
    // measurement build: wide 300-d batches on the id set with partial-distance early abandon after k blocks (dist_rounds_inflight)
    if (plan.walk == SearchWalk::OnChipIds && knobs.ea > 0 && ix->L.nb == 9 && ix->L.rs == 1 && ix->L.tail == 1) {
#define EA_CASE(K_)                                                                                   \
    case K_: {                                                                                        \
        auto kS = search_kernel<9, 1, 1, walk_with_ea(kWalkFatIds, K_)>;                              \
        IDIST_LAUNCH(kS, grid, 64, smem, stream, view, a);                                            \
        break;                                                                                        \
    }
        switch (knobs.ea) {
            EA_CASE(4) EA_CASE(5) EA_CASE(6) EA_CASE(7)
            default: return fail(IDIST_ERR_INVALID_ARG, "IDIST_EA=%d: 4..7", knobs.ea);
        }
#undef EA_CASE
    } else
#endif
    IDIST_DISPATCH(ix->L, LAUNCH_SEARCH);
#undef LAUNCH_SEARCH
#undef SEARCH_CASE
#undef IDIST_VARIANT_SEARCH_CASES
    if (!launched) return fail(IDIST_ERR_INTERNAL, "no search kernel for the walk %s at this row geometry (stride %u)", walk_name(plan.walk), ix->L.stride);
    if (const hipError_t le = hipGetLastError(); le != hipSuccess) {
        // nothing ran: put the queue head back where a fresh context has it
        hipMemsetAsync(ctx->d_next, 0, 4, stream);
        ctx->queue_base = 0;
        return fail(IDIST_ERR_HIP, "search launch failed: %s", hipGetErrorString(le));
    }
    ctx->queue_base += nq + grid;
    if (knobs.events) {
        HIPCHK(hipEventRecord(ctx->ev1[slot], stream));
        ctx->n_launch++;
        ctx->recs[ctx->n_rec++ % IDIST_EVENT_RING] = {(int32_t)slot, 0.0f};
    }
    if (passes) CHK(metric.report(d_dist, ctx->d_sq, nq, ef, stream));
    return IDIST_OK;
}

}  // namespace

extern "C" {

const char* idist_last_error(void) { return g_err.c_str(); }
const char* idist_version(void) { return "instant-distance_amd 0.1 (gfx950)"; }

idist_status idist_device_count(int32_t* out) {
    if (!out) return fail(IDIST_ERR_INVALID_ARG, "out is null");
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) cnt = 0;
    *out = cnt;
    return IDIST_OK;
}

idist_status idist_default_config(idist_config* cfg) {   // core/lib.rs:101-128
    if (!cfg) return fail(IDIST_ERR_INVALID_ARG, "cfg is null");
    cfg->ef_search = 100;
    cfg->ef_construction = 100;
    cfg->ml = 1.0f / logf((float)IDIST_M);
    cfg->has_heuristic = 1;
    cfg->extend_candidates = 0;
    cfg->keep_pruned = 1;
    cfg->metric = IDIST_METRIC_L2SQ;
    cfg->max_batch = 0;
    cfg->tie_policy = IDIST_TIES_STRICT;
    cfg->tie_capacity = 0;
    cfg->dot_bound = 0.0f;
    return IDIST_OK;
}

idist_status idist_layer_sizes(uint32_t n, float ml, uint32_t* cum, uint32_t cap, uint32_t* n_layers) {
    if (!cum || !n_layers) return fail(IDIST_ERR_INVALID_ARG, "null output");
    uint32_t tmp[IDIST_MAX_LAYERS + 1];
    const uint32_t nl = n ? layer_sizes(n, ml, tmp, IDIST_MAX_LAYERS) : 0;
    if (n && nl == 0) return fail(IDIST_ERR_INVALID_ARG, "more than %u layers", IDIST_MAX_LAYERS);
    if (nl > cap) return fail(IDIST_ERR_INVALID_ARG, "cum holds %u entries, %u needed", cap, nl);
    for (uint32_t i = 0; i < nl; i++) cum[i] = tmp[i];
    *n_layers = nl;
    return IDIST_OK;
}

idist_status idist_permutation(uint64_t seed, uint32_t n, uint32_t* out_pid, uint32_t* order) {
    // SmallRng (xoshiro256++) seeded through SplitMix64; PARITY UNPINNED, see idist.h
    uint64_t st = seed, s[4];
    for (int i = 0; i < 4; i++) {
        uint64_t z = (st += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        s[i] = z ^ (z >> 31);
    }
    auto rotl = [](uint64_t x, int k) { return (x << k) | (x >> (64 - k)); };
    auto next_u32 = [&]() {
        const uint64_t result = rotl(s[0] + s[3], 23) + s[0];
        const uint64_t t = s[1] << 17;
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3];
        s[2] ^= t; s[3] = rotl(s[3], 45);
        return (uint32_t)(result >> 32);
    };
    std::vector<std::pair<uint32_t, uint32_t>> sh(n);
    for (uint32_t i = 0; i < n; i++) {                       // core/lib.rs:257-259
        const uint64_t m = (uint64_t)next_u32() * n;
        uint32_t key = (uint32_t)(m >> 32);
        const uint32_t lo = (uint32_t)m;
        if (lo > (uint32_t)(0u - n)) {
            const uint32_t hi2 = (uint32_t)(((uint64_t)next_u32() * n) >> 32);
            if ((uint64_t)lo + hi2 > 0xFFFFFFFFull) key += 1;
        }
        sh[i] = {key, i};
    }
    std::sort(sh.begin(), sh.end());                         // sort_unstable, :260 (all pairs distinct)
    for (uint32_t i = 0; i < n; i++) {                       // :262-270
        if (out_pid) out_pid[sh[i].second] = i;
        if (order) order[i] = sh[i].second;
    }
    return IDIST_OK;
}

idist_status idist_index_build(const float* points, uint32_t n, uint32_t dim, const idist_config* cfg,
                               int32_t device, idist_index** out) {
    if (!out) return fail(IDIST_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    return build_common(points, false, n, dim, cfg, device, out);
}

idist_status idist_index_build_device(const void* d_points, uint32_t n, uint32_t dim, const idist_config* cfg,
                                      int32_t device, idist_index** out) {
    if (!out) return fail(IDIST_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    return build_common(d_points, true, n, dim, cfg, device, out);
}

idist_status idist_progress_new(idist_progress** out) {
    if (!out) return fail(IDIST_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    idist_progress* p = new idist_progress();
    void* m = nullptr;
    hipError_t e = hipHostMalloc(&m, 64, hipHostMallocPortable | hipHostMallocMapped);
    if (e != hipSuccess) { delete p; return fail(IDIST_ERR_HIP, "hipHostMalloc(progress): %s", hipGetErrorString(e)); }
    p->slot = reinterpret_cast<volatile unsigned long long*>(m);
    p->slot[0] = 0;
    p->slot[1] = 0;
    *out = p;
    return IDIST_OK;
}

void idist_progress_free(idist_progress* p) {
    if (!p) return;
    if (g_watch == p) g_watch = nullptr;
    if (p->slot) hipHostFree(const_cast<unsigned long long*>(p->slot));
    delete p;
}

idist_status idist_progress_watch_next_build(idist_progress* p) {
    g_watch = p;
    return IDIST_OK;
}

idist_status idist_progress_get(const idist_progress* p, uint64_t* done, uint64_t* total, int32_t* layer) {
    if (!p) return fail(IDIST_ERR_INVALID_ARG, "progress is null");
    if (done) *done = p->slot[0];
    if (total) *total = p->total;
    if (layer) *layer = (int32_t)p->slot[1] - 1;
    return IDIST_OK;
}

idist_status idist_index_build_stats(const idist_index* idx, idist_build_stats* out) {
    if (!idx || !out) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    *out = idx->stats;
    return IDIST_OK;
}

idist_status idist_index_import(const float* points, uint32_t n, uint32_t dim, const idist_config* cfg,
                                const uint32_t* zero, const uint32_t* const* layers, const uint32_t* layer_len,
                                uint32_t n_upper, int32_t device, idist_index** out) {
    if (!out) return fail(IDIST_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    CHK(validate_config(cfg, false));
    if (n && (!points || !zero)) return fail(IDIST_ERR_INVALID_ARG, "points/zero is null");
    if (n_upper && (!layers || !layer_len)) return fail(IDIST_ERR_INVALID_ARG, "layers/layer_len is null");
    for (uint32_t l = 0; l < n_upper; l++)
        if (layer_len[l] == 0 || layer_len[l] > n || (l && layer_len[l] > layer_len[l - 1]))
            return fail(IDIST_ERR_BAD_GRAPH, "layer_len[%u] = %u: layers must nest (core/lib.rs:323-327)", l, layer_len[l]);
    idist_index* ix = nullptr;
    CHK(index_alloc(n, dim, cfg, layer_len, n_upper, device, &ix));
    auto bail = [&](idist_status s) { idist_index_free(ix); return s; };
    idist_status s = load_points_host(ix, points);
    if (s != IDIST_OK) return bail(s);
    if (n) {
        if (hipMemcpy(ix->d_zero, zero, (size_t)n * IDIST_M2 * 4, hipMemcpyHostToDevice) != hipSuccess)
            return bail(fail(IDIST_ERR_HIP, "hipMemcpy(zero) failed"));
        for (uint32_t l = 0; l < n_upper; l++)
            if (hipMemcpy(ix->d_upper + ix->layer_off[l] * IDIST_M, layers[l], (size_t)layer_len[l] * IDIST_M * 4,
                          hipMemcpyHostToDevice) != hipSuccess)
                return bail(fail(IDIST_ERR_HIP, "hipMemcpy(layer %u) failed", l + 1));
        // validate against the reference's invariants
        uint32_t* d_bad = nullptr;
        if (hipMalloc((void**)&d_bad, 256) != hipSuccess || hipMemset(d_bad, 0, 256) != hipSuccess)
            return bail(fail(IDIST_ERR_HIP, "hipMalloc(validate) failed"));
        IDIST_LAUNCH(validate_rows_kernel, std::min<uint32_t>(n, 8192), 64, 0, (hipStream_t) nullptr, ix->d_zero, n, kM2, n, d_bad);
        for (uint32_t l = 0; l < n_upper; l++)
            IDIST_LAUNCH(validate_rows_kernel, std::min<uint32_t>(layer_len[l], 8192), 64, 0, (hipStream_t) nullptr,
                         ix->d_upper + ix->layer_off[l] * IDIST_M, layer_len[l], kM, layer_len[l], d_bad);
        uint32_t bad = 0;
        hipError_t e = hipMemcpy(&bad, d_bad, 4, hipMemcpyDeviceToHost);
        hipFree(d_bad);
        if (e != hipSuccess) return bail(fail(IDIST_ERR_HIP, "validate: %s", hipGetErrorString(e)));
        if (bad)
            return bail(fail(IDIST_ERR_BAD_GRAPH,
                             "%u adjacency rows hold an id outside their layer or a duplicate id", bad));
    }
    *out = ix;
    return IDIST_OK;
}

idist_status idist_index_alloc(uint32_t n, uint32_t dim, const idist_config* cfg, const uint32_t* layer_len,
                               uint32_t n_upper, int32_t device, idist_index** out) {
    CHK(validate_config(cfg, false));
    if (n_upper && !layer_len) return fail(IDIST_ERR_INVALID_ARG, "layer_len is null");
    // the rows this index will be filled with already are x~: the S they were made with has to come with them
    if (is_dot(*cfg) && !(cfg->dot_bound > 0.0f))
        return fail(IDIST_ERR_INVALID_ARG, "an inner-product replication target needs the source's dot_bound (idist_index_get_info), got 0");
    return index_alloc(n, dim, cfg, layer_len, n_upper, device, out);
}

idist_status idist_index_export(const idist_index* idx, uint32_t* zero, uint32_t* const* layers) {
    if (!idx) return fail(IDIST_ERR_INVALID_ARG, "idx is null");
    HIPCHK(hipSetDevice(idx->device));
    if (idx->n) {
        if (!zero) return fail(IDIST_ERR_INVALID_ARG, "zero is null");
        HIPCHK(hipMemcpy(zero, idx->d_zero, (size_t)idx->n * IDIST_M2 * 4, hipMemcpyDeviceToHost));
    }
    for (uint32_t l = 0; l < idx->n_upper; l++) {
        if (!layers || !layers[l]) return fail(IDIST_ERR_INVALID_ARG, "layers[%u] is null", l);
        HIPCHK(hipMemcpy(layers[l], idx->d_upper + idx->layer_off[l] * IDIST_M, (size_t)idx->layer_len[l] * IDIST_M * 4,
                         hipMemcpyDeviceToHost));
    }
    return IDIST_OK;
}

idist_status idist_index_get_info(const idist_index* idx, idist_index_info* out) {
    if (!idx || !out) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    memset(out, 0, sizeof(*out));
    out->n = idx->n;
    out->dim = idx->dim;
    out->row_stride = idx->L.stride;
    out->n_upper = idx->n_upper;
    out->ef_search = idx->cfg.ef_search;
    out->metric = idx->cfg.metric;
    out->device = idx->device;
    out->tie_capacity = tie_capacity(idx->cfg);
    out->dot_bound = is_dot(idx->cfg) ? idx->dot_S : 0.0f;
    for (uint32_t l = 0; l < idx->n_upper; l++) out->layer_len[l] = idx->layer_len[l];
    // the reject filter's tables are made on first use (a wide search, idist_filter_bound_batch, a build): NONE / 0 / 0 until then —
    // asking must not make them, the rows of a replication target may not have arrived yet
    if (idx->filt_state.load(std::memory_order_acquire) == 1) {
        out->filter_bytes = (uint64_t)idx->n * idx->filt.fstride;
        if (idx->filt_p_state.load(std::memory_order_acquire) == 1) {       // (the format is decided: nothing below is written again)
            out->filter_format = idx->filt_format.load(std::memory_order_relaxed);
            out->filter_principal_bytes = idx->filt_p.rows ? (uint64_t)idx->n * idx->filt_p.fstride : 0u;
            if (idx->filt_inl_state.load(std::memory_order_acquire) == 1) out->filter_inline_bytes = (uint64_t)idx->n * idist::kInlineBlockBytes;
        }
    }
    return IDIST_OK;
}

idist_status idist_index_device_buffers(const idist_index* idx, idist_device_buffers* out) {
    if (!idx || !out) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    out->points = idx->d_points;
    out->points_bytes = (size_t)idx->n * idx->L.stride * 4;
    out->zero = idx->d_zero;
    out->zero_bytes = (size_t)idx->n * IDIST_M2 * 4;
    out->upper = idx->d_upper;
    out->upper_bytes = idx->upper_rows * IDIST_M * 4;
    return IDIST_OK;
}

idist_status idist_index_set_ef_search(idist_index* idx, uint32_t ef_search) {
    if (!idx) return fail(IDIST_ERR_INVALID_ARG, "idx is null");
    if (ef_search > IDIST_MAX_EF) return fail(IDIST_ERR_INVALID_ARG, "ef_search %u > %u", ef_search, IDIST_MAX_EF);
    idx->cfg.ef_search = ef_search;
    return IDIST_OK;
}

void idist_index_free(idist_index* idx) {
    if (!idx) return;
    hipSetDevice(idx->device);
    for (idist_search_ctx* c : idx->comb_ctx) idist_search_ctx_free(c);
    hipFree(idx->d_points);
    hipFree(idx->d_zero);
    hipFree(idx->d_upper);
    hipFree(idx->d_layer_off);
    hipFree(const_cast<uint8_t*>(idx->filt.rows));
    hipFree(const_cast<uint8_t*>(idx->filt_p.rows));
    hipFree(const_cast<float*>(idx->filt_p.basis));
    hipFree(const_cast<float*>(idx->filt_p.mu));
    hipFree(idx->filt_inl);
    delete idx;
}

idist_status idist_search_ctx_new(const idist_index* idx, uint32_t slots, idist_search_ctx** out) {
    if (!idx || !out) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    HIPCHK(hipSetDevice(idx->device));
    idist_search_ctx* c = new idist_search_ctx();
    c->idx = idx;
    c->idx_uid = idx->uid;
    c->slots_req = slots;
    c->vis = vis_geometry(idx->n);
    c->knobs = knobs_from_env();
    c->tie_policy = idx->cfg.tie_policy;
    c->base_tie_cap = tie_capacity(idx->cfg);
    c->n_points = idx->n;
    c->stride = idx->L.stride;
    c->device = idx->device;
    c->n_cu = idx->n_cu;
    auto bail = [&](hipError_t e) {
        idist_search_ctx_free(c);
        return fail(IDIST_ERR_HIP, "search ctx allocation failed: %s", hipGetErrorString(e));
    };
    hipError_t e;
    if ((e = hipMalloc((void**)&c->d_next, 256)) != hipSuccess) return bail(e);
    if ((e = hipMemset(c->d_next, 0, 256)) != hipSuccess) return bail(e);
    if ((e = hipStreamCreate(&c->stream)) != hipSuccess) return bail(e);
    for (uint32_t i = 0; i < IDIST_EVENT_RING; i++) {
        if ((e = hipEventCreate(&c->ev0[i])) != hipSuccess) return bail(e);
        if ((e = hipEventCreate(&c->ev1[i])) != hipSuccess) return bail(e);
    }
    // Search::default() is cheap (core/lib.rs:767-778): one slot = n/8 bytes now; the bitmaps of further slots
    // are allocated when a batch first needs them (ensure_slots), or right away if the caller named a count
    if (ensure_slots(c, slots ? slots : 1u, nullptr) != IDIST_OK) { idist_search_ctx_free(c); return IDIST_ERR_HIP; }
    // the scratch above was cleared on the null stream; a caller's non-blocking stream would not wait for it
    if ((e = hipStreamSynchronize(nullptr)) != hipSuccess) return bail(e);
    *out = c;
    return IDIST_OK;
}

void idist_search_ctx_free(idist_search_ctx* c) {
    if (!c) return;
    // (the index may already be gone: nothing of it is touched here)
    hipFree(c->d_visited);
    hipFree(c->d_tie_spill);
    hipFree(c->d_next);
    if (c->h_io) hipHostFree(c->h_io);
    for (hipEvent_t e : c->al_ev)
        if (e) hipEventDestroy(e);
    for (hipEvent_t e : c->at_ev)
        if (e) hipEventDestroy(e);
    for (uint32_t i = 0; i < IDIST_EVENT_RING; i++) {
        if (c->ev0[i]) hipEventDestroy(c->ev0[i]);
        if (c->ev1[i]) hipEventDestroy(c->ev1[i]);
    }
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;                      // the staging (every DevBuf) goes here, after its stream: hipFree synchronises the device
}

idist_status idist_search_ctx_reserve(idist_search_ctx* ctx, uint32_t slots) {
    if (!ctx) return fail(IDIST_ERR_INVALID_ARG, "ctx is null");
    // the bitmaps belong on the context's own device whatever device the calling thread has current (replicas on several
    // GPUs); device, CU count and point count were copied at creation — the index itself is not touched (it may be gone)
    HIPCHK(hipSetDevice(ctx->device));
    const uint32_t cap = ctx->slots_req ? ctx->slots_req : 0xFFFFFFFFu;
    CHK(ensure_slots(ctx, std::min(std::max(slots, 1u), cap), ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));                   // the new bitmaps are cleared before any stream may use them
    return IDIST_OK;
}

// prepared: see SearchOpts (the partitioned search hands in what the kernels read and reports the distances after its merge)
static idist_status search_batch_device_impl(const idist_index* idx, idist_search_ctx* ctx, const void* d_queries,
                                             uint32_t nq, void* d_out_pid, void* d_out_dist, void* d_out_count,
                                             void* d_out_counters, void* hip_stream, bool prepared) {
    CHK(check_ctx(idx, ctx));
    if (nq == 0) return IDIST_OK;
    if (!d_queries || !d_out_count) return fail(IDIST_ERR_INVALID_ARG, "null device pointer");
    HIPCHK(hipSetDevice(idx->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    if (idx->n == 0 || idx->cfg.ef_search == 0) {   // core/lib.rs:359-361
        HIPCHK(hipMemsetAsync(d_out_count, 0, (size_t)nq * 4, stream));
        return IDIST_OK;
    }
    if (!d_out_pid || !d_out_dist) return fail(IDIST_ERR_INVALID_ARG, "null device pointer");
    SearchOpts opts;
    opts.prepared = prepared;
    return launch_search(idx, ctx, (const float*)d_queries, nq, (uint32_t*)d_out_pid, (float*)d_out_dist,
                         (uint32_t*)d_out_count, (uint32_t*)d_out_counters, stream, opts);
}

idist_status idist_search_batch_device(const idist_index* idx, idist_search_ctx* ctx, const void* d_queries,
                                       uint32_t nq, void* d_out_pid, void* d_out_dist, void* d_out_count,
                                       void* d_out_counters, void* hip_stream) {
    return search_batch_device_impl(idx, ctx, d_queries, nq, d_out_pid, d_out_dist, d_out_count, d_out_counters, hip_stream, false);
}

idist_status idist_search_ctx_status(idist_search_ctx* ctx) {
    if (!ctx) return fail(IDIST_ERR_INVALID_ARG, "ctx is null");
    uint32_t st = 0;
    HIPCHK(hipMemcpy(&st, ctx->d_next + 1, 4, hipMemcpyDeviceToHost));
    if (st) HIPCHK(hipMemset(ctx->d_next + 1, 0, 4));
    if (st & kStTieOverflow) {
        ctx->tie_overflowed = true;
        // strict: later launches of this context get a larger tie region (x4, at most 4096 entries, LDS permitting); when that
        // is exhausted, HBM bags that take whatever the region cannot (unbounded, like the reference's heap)
        const uint32_t cap = std::max(ctx->base_tie_cap, ctx->tie_cap), next = std::min<uint32_t>(4096u, cap * 4u);
        if (ctx->tie_policy == IDIST_TIES_STRICT) {
            if (!ctx->knobs.tie_spill_first && next > cap &&
                smem_bytes(ctx->stride, ctx->last_ef + 64 + next + 8, false, kBloomWords, ctx->vis.dirty_words) <= 64 * 1024)
                ctx->tie_cap = next;
            else if (!ctx->tie_spill) ctx->tie_spill = true;
            else ctx->tie_escalation_exhausted = true;
        }
        g_tie_cap_msg = cap;
    }
    return device_status_to_code(st, ctx->tie_policy);
}

idist_status idist_search_ctx_filter_principal_counts(idist_search_ctx* ctx, uint64_t* examined, uint64_t* rejected, int32_t reset) {
    if (!ctx) return fail(IDIST_ERR_INVALID_ARG, "ctx is null");
    unsigned long long c[2] = {0, 0};
    HIPCHK(hipMemcpy(c, ctx->d_next + 20, sizeof(c), hipMemcpyDeviceToHost));
    if (reset) HIPCHK(hipMemset(ctx->d_next + 20, 0, sizeof(c)));
    if (examined) *examined = c[0];
    if (rejected) *rejected = c[1];
    return IDIST_OK;
}

idist_status idist_search_ctx_filter_inline_counts(idist_search_ctx* ctx, uint64_t* blocks_requested, uint64_t* blocks_used, int32_t reset) {
    if (!ctx) return fail(IDIST_ERR_INVALID_ARG, "ctx is null");
    unsigned long long c[2] = {0, 0};
    HIPCHK(hipMemcpy(c, ctx->d_next + 24, sizeof(c), hipMemcpyDeviceToHost));
    if (reset) HIPCHK(hipMemset(ctx->d_next + 24, 0, sizeof(c)));
    if (blocks_requested) *blocks_requested = c[0];
    if (blocks_used) *blocks_used = c[1];
    return IDIST_OK;
}

idist_status idist_search_ctx_filter_counts(idist_search_ctx* ctx, uint64_t* examined, uint64_t* rejected, int32_t reset) {
    if (!ctx) return fail(IDIST_ERR_INVALID_ARG, "ctx is null");
    unsigned long long c[2] = {0, 0};
    HIPCHK(hipMemcpy(c, ctx->d_next + 16, sizeof(c), hipMemcpyDeviceToHost));   // (waits for the null stream only: synchronise first)
    if (reset) HIPCHK(hipMemset(ctx->d_next + 16, 0, sizeof(c)));
    if (examined) *examined = c[0];
    if (rejected) *rejected = c[1];
    return IDIST_OK;
}

idist_status idist_search_ctx_tie_overflowed(idist_search_ctx* ctx, int32_t* out) {
    if (!ctx || !out) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    CHK(idist_search_ctx_status(ctx));
    *out = ctx->tie_overflowed ? 1 : 0;
    ctx->tie_overflowed = false;
    return IDIST_OK;
}

// Reads the context's device-side status behind a launch (*st).  True: strict ties overflowed and the escalation made progress —
// idist_search_ctx_status gave this context a larger tie region or the HBM bags — so the batch is simply searched again (queries
// are independent and the results are overwritten).
static bool status_asks_retry(const idist_index* idx, idist_search_ctx* ctx, idist_status* st) {
    const uint32_t cap_before = std::max(tie_capacity(idx->cfg), ctx->tie_cap);
    const bool spill_before = ctx->tie_spill;
    *st = idist_search_ctx_status(ctx);
    return *st == IDIST_ERR_TIE_OVERFLOW && (std::max(tie_capacity(idx->cfg), ctx->tie_cap) > cap_before || ctx->tie_spill != spill_before);
}

static idist_status resolve_time(idist_search_ctx* ctx, const idist_search_ctx::TimeRec& r, float* ms) {
    if (r.slot < 0) { *ms = r.ms; return IDIST_OK; }
    HIPCHK(hipEventSynchronize(ctx->ev1[r.slot]));
    HIPCHK(hipEventElapsedTime(ms, ctx->ev0[r.slot], ctx->ev1[r.slot]));
    return IDIST_OK;
}

idist_status idist_search_ctx_last_kernel_ms(idist_search_ctx* ctx, float* ms) {
    if (!ctx || !ms) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    if (!ctx->n_rec) return fail(IDIST_ERR_INVALID_ARG, "no search kernel has been timed for this ctx (IDIST_KERNEL_EVENTS=0, or no call yet)");
    return resolve_time(ctx, ctx->recs[(ctx->n_rec - 1) % IDIST_EVENT_RING], ms);
}

idist_status idist_search_ctx_kernel_times(idist_search_ctx* ctx, float* ms, uint32_t cap, uint32_t* n_out) {
    if (!ctx || !ms || !n_out) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    const uint64_t have = std::min<uint64_t>(ctx->n_rec, IDIST_EVENT_RING);
    const uint32_t take = (uint32_t)std::min<uint64_t>(have, cap);
    for (uint32_t i = 0; i < take; i++) CHK(resolve_time(ctx, ctx->recs[(ctx->n_rec - take + i) % IDIST_EVENT_RING], &ms[i]));
    *n_out = take;
    return IDIST_OK;
}

static idist_status search_batch_impl(const idist_index* idx, idist_search_ctx* ctx, const float* queries, uint32_t nq,
                                      uint32_t* out_pid, float* out_dist, uint32_t* out_count, uint32_t* out_counters);

// A leader's launch for the scalar calls it took along (idist_combine.hpp).  Alone: on the leader's own context.  With
// company: on its slot's context, which grows with the batches (the leader's own may be a one-slot `Search`).
static void run_combined(const idist_index* idx, idist_search_ctx* ctx, std::vector<ScalarReq*>& b, int slot) {
    const uint32_t k = (uint32_t)b.size(), ef = idx->cfg.ef_search, dim = idx->dim;
    idist_status st = IDIST_OK;
    if (k == 1) {
        st = search_batch_impl(idx, ctx, b[0]->q, 1, b[0]->pid, b[0]->dist, b[0]->cnt, b[0]->ctr);
    } else if (!idx->comb_ctx[slot] && (st = idist_search_ctx_new(idx, kCombineBatch, &idx->comb_ctx[slot])) != IDIST_OK) {   // backed for a full batch at once: growing a context later would synchronise the device under everybody's feet
        // (reported to every caller of the batch below)
    } else {
        ctx = idx->comb_ctx[slot];
        std::vector<float> q((size_t)k * dim), dd((size_t)k * ef);
        std::vector<uint32_t> pid((size_t)k * ef), cnt(k), ctr((size_t)k * 3);
        for (uint32_t i = 0; i < k; i++) memcpy(q.data() + (size_t)i * dim, b[i]->q, (size_t)dim * 4);
        st = search_batch_impl(idx, ctx, q.data(), k, pid.data(), dd.data(), cnt.data(), ctr.data());
        if (st == IDIST_OK)
            for (uint32_t i = 0; i < k; i++) {
                memcpy(b[i]->pid, pid.data() + (size_t)i * ef, (size_t)ef * 4);
                memcpy(b[i]->dist, dd.data() + (size_t)i * ef, (size_t)ef * 4);
                b[i]->cnt[0] = cnt[i];
                if (b[i]->ctr) memcpy(b[i]->ctr, ctr.data() + (size_t)i * 3, 12);
            }
    }
    float kms = -1.0f;
    if (st == IDIST_OK && k > 1 && ctx->n_rec) (void)resolve_time(ctx, ctx->recs[(ctx->n_rec - 1) % IDIST_EVENT_RING], &kms);
    for (ScalarReq* r : b) {
        r->st = st;
        r->kernel_ms = kms;
        if (st != IDIST_OK) r->err = g_err;
    }
}

idist_status idist_search_batch(const idist_index* idx, idist_search_ctx* ctx, const float* queries, uint32_t nq,
                                uint32_t* out_pid, float* out_dist, uint32_t* out_count, uint32_t* out_counters) {
    CHK(check_ctx(idx, ctx));
    if (nq == 0) return IDIST_OK;
    if (!queries || !out_count) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    const uint32_t ef = idx->cfg.ef_search;
    if (idx->n == 0 || ef == 0) {
        memset(out_count, 0, (size_t)nq * 4);
        if (out_counters) memset(out_counters, 0, (size_t)nq * 12);
        return IDIST_OK;
    }
    if (!out_pid || !out_dist) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    // The reference's scalar call, possibly from many threads at once (one Search each, core/lib.rs:352-356): beyond eight
    // launches in flight on this index a call rides along in another thread's launch instead of making its own
    // (IDIST_TIES_DROP: idist_search_ctx_tie_overflowed is a per-context answer about the caller's OWN queries — such calls
    // always launch on their own context.  Strict ties: where the escalated region / the bags live is unobservable.)
    if (nq == 1 && ctx->knobs.combine && idx->cfg.tie_policy != IDIST_TIES_DROP) {
        ScalarReq r{queries, out_pid, out_dist, out_count, out_counters};
        idx->comb.submit(r, [&](std::vector<ScalarReq*>& b, int slot) { run_combined(idx, ctx, b, slot); });
        if (r.st != IDIST_OK) g_err = r.err;
        // a call that rode along (or led company) ran on a slot context: its kernel time is reported through the caller's own
        else if (r.kernel_ms >= 0.0f) ctx->recs[ctx->n_rec++ % IDIST_EVENT_RING] = {-1, r.kernel_ms};
        return r.st;
    }
    return search_batch_impl(idx, ctx, queries, nq, out_pid, out_dist, out_count, out_counters);
}

static idist_status search_batch_impl(const idist_index* idx, idist_search_ctx* ctx, const float* queries, uint32_t nq,
                                      uint32_t* out_pid, float* out_dist, uint32_t* out_count, uint32_t* out_counters) {
    const uint32_t ef = idx->cfg.ef_search;
    HIPCHK(hipSetDevice(idx->device));
    const size_t qb = (size_t)nq * idx->dim * 4, ob = (size_t)nq * ef * 4;
    // Narrow batches — the reference's call is ONE query per Hnsw::search: query and results cross PCIe through one
    // pinned, device-mapped buffer that the kernel reads and writes itself; the call is a host memcpy, one launch, one
    // stream sync, a host memcpy.  (The general path below costs six copy / memset calls of ~10 us each around the kernel.)
    const size_t io_need = qb + 2 * ob + (size_t)nq * 16 + idist_search_ctx::kIoHeadBytes;
    // (not for a metric with passes: the completion word the kernel writes would run ahead of the pass behind the walk)
    if (io_need <= idist_search_ctx::kIoMaxBytes && !ctx->knobs.no_zero_copy && !MetricPasses(idx).any()) {
        if (io_need > ctx->io_cap) {
            size_t cap = idist_search_ctx::kIoMinBytes;
            while (cap < io_need) cap <<= 1;
            HIPCHK(hipStreamSynchronize(ctx->stream));
            if (ctx->h_io) hipHostFree(ctx->h_io);
            ctx->h_io = nullptr;
            ctx->io_cap = 0;
            // coherent (fine-grained) on purpose: the host polls the completion word and reads the results WHILE the stream is
            // still busy — with a non-coherent mapping (HIP_HOST_COHERENT=0) they would only be visible at kernel end
            HIPCHK(hipHostMalloc((void**)&ctx->h_io, cap, hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent));
            if (hipHostGetDevicePointer((void**)&ctx->d_io, ctx->h_io, 0) != hipSuccess) ctx->d_io = ctx->h_io;
            ctx->io_cap = cap;
        }
        uint8_t* hp = ctx->h_io;
        uint32_t* h_status = (uint32_t*)hp;                                   // [256]
        volatile uint32_t* h_done = (volatile uint32_t*)(hp + idist_search_ctx::kIoStatusSlots * 4);   // completion word
        float* h_q = (float*)(hp + idist_search_ctx::kIoHeadBytes);
        uint32_t* h_pid = (uint32_t*)((uint8_t*)h_q + qb);
        float* h_dist = (float*)((uint8_t*)h_pid + ob);
        uint32_t* h_cnt = (uint32_t*)((uint8_t*)h_dist + ob);
        uint32_t* h_ctr = h_cnt + nq;
        const ptrdiff_t dv = ctx->d_io - ctx->h_io;                           // host address -> device address of the same byte
        for (;;) {
            memcpy(h_q, queries, qb);
            memset(h_status, 0, idist_search_ctx::kIoStatusSlots * 4);
            *h_done = 0u;
            uint32_t grid = 0;
            const bool flag = ctx->knobs.sync_flag;
            const uint32_t seq = ++ctx->done_seq ? ctx->done_seq : ++ctx->done_seq;       // never 0: a fresh buffer reads 0
            const auto t0 = std::chrono::steady_clock::now();
            SearchOpts opts;
            opts.status_host = (uint32_t*)((uint8_t*)h_status + dv);
            opts.grid_out = &grid;
            opts.done_host = flag ? (uint32_t*)((uint8_t*)h_done + dv) : nullptr;
            opts.done_seq = seq;
            CHK(launch_search(idx, ctx, (const float*)((uint8_t*)h_q + dv), nq, (uint32_t*)((uint8_t*)h_pid + dv),
                              (float*)((uint8_t*)h_dist + dv), (uint32_t*)((uint8_t*)h_cnt + dv),
                              out_counters ? (uint32_t*)((uint8_t*)h_ctr + dv) : nullptr, ctx->stream, opts));
            if (flag) {
                // The kernel's last workgroup writes `seq` into the pinned buffer behind its results.  One Search per thread
                // is the reference's model, so waiting must not burn a core per thread: sleep through the first half of what
                // such a call has been taking, then poll the word; a stream synchronisation only if it stays away for 2 s.
                bool overslept = false;
                if (ctx->call_ns_ema > 200e3) {
                    struct timespec ts = {0, (long)(ctx->call_ns_ema * 0.5)};
                    nanosleep(&ts, nullptr);
                    overslept = *h_done == seq;                       // done before we looked: the estimate is too long
                }
                bool seen = false;
                for (uint64_t spins = 0; !(seen = (*h_done == seq)); spins++) {
                    if (spins < 2048u) cpu_relax();
                    else std::this_thread::yield();               // 64+ waiting threads must not keep the leaders off the cores
                    if ((spins & 0x3FFFu) == 0x3FFFu &&
                        std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 2.0) break;
                }
                std::atomic_thread_fence(std::memory_order_acquire);
                if (!seen) HIPCHK(hipStreamSynchronize(ctx->stream));
                const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
                if (overslept) ctx->call_ns_ema *= 0.7;
                else if (ctx->n_flag_calls++ > 0)                     // (the first call also allocated: not a sample)
                    ctx->call_ns_ema = ctx->call_ns_ema == 0.0 ? ns : 0.8 * ctx->call_ns_ema + 0.2 * ns;
            } else {
                HIPCHK(hipStreamSynchronize(ctx->stream));
            }
            uint32_t any = grid <= idist_search_ctx::kIoStatusSlots ? 0u : 1u;  // too many workgroups for the slots: ask the device
            for (uint32_t g = 0; g < grid && g < idist_search_ctx::kIoStatusSlots; g++) any |= h_status[g];
            if (any) {
                idist_status s;
                if (status_asks_retry(idx, ctx, &s)) continue;
                if (s != IDIST_OK) return s;
            }
            memcpy(out_pid, h_pid, ob);
            memcpy(out_dist, h_dist, ob);
            memcpy(out_count, h_cnt, (size_t)nq * 4);
            if (out_counters) memcpy(out_counters, h_ctr, (size_t)nq * 12);
            return IDIST_OK;
        }
    }
    CHK(ctx->d_q.grow(qb));
    CHK(ctx->d_pid.grow(ob));
    CHK(ctx->d_dist.grow(ob));
    CHK(ctx->d_cnt.grow((size_t)nq * 4));
    CHK(ctx->d_ctr.grow((size_t)nq * 12));
    HIPCHK(hipMemcpyAsync(ctx->d_q, queries, qb, hipMemcpyHostToDevice, ctx->stream));
    for (;;) {
        CHK(launch_search(idx, ctx, ctx->d_q, nq, ctx->d_pid, ctx->d_dist, ctx->d_cnt, out_counters ? ctx->d_ctr.p : nullptr,
                          ctx->stream));
        HIPCHK(hipMemcpyAsync(out_pid, ctx->d_pid, ob, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(out_dist, ctx->d_dist, ob, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(out_count, ctx->d_cnt, (size_t)nq * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (out_counters) HIPCHK(hipMemcpyAsync(out_counters, ctx->d_ctr, (size_t)nq * 12, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        idist_status s;
        if (!status_asks_retry(idx, ctx, &s)) return s;
    }
}

// ---- several GPUs of one node: replicate once, shard the queries ----
idist_status idist_replicate(const idist_index* root, const int32_t* devices, uint32_t n_devices, idist_index** replicas) {
    if (!root || !replicas || (n_devices && !devices)) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    for (uint32_t i = 0; i < n_devices; i++) replicas[i] = nullptr;
    auto undo = [&](idist_status s) {
        const std::string keep = g_err;
        for (uint32_t i = 0; i < n_devices; i++) { idist_index_free(replicas[i]); replicas[i] = nullptr; }
        hipSetDevice(root->device);
        g_err = keep;
        return s;
    };
    std::vector<hipStream_t> streams(n_devices, nullptr);
    auto drop_streams = [&]() {
        for (uint32_t i = 0; i < n_devices; i++)
            if (streams[i]) { hipSetDevice(devices[i]); hipStreamDestroy(streams[i]); }
    };
    const size_t pb = (size_t)root->n * root->L.stride * 4, zb = (size_t)root->n * IDIST_M2 * 4, ub = root->upper_rows * IDIST_M * 4;
    // make sure nothing is still writing the root's buffers (a build on another stream)
    if (hipSetDevice(root->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return fail(IDIST_ERR_HIP, "replicate: root device %d: %s", root->device, hipGetErrorString(hipGetLastError()));
    for (uint32_t i = 0; i < n_devices; i++) {
        idist_index* r = nullptr;
        idist_status st = index_alloc(root->n, root->dim, &root->cfg, root->layer_len, root->n_upper, devices[i], &r);   // sets the device
        if (st != IDIST_OK) { drop_streams(); return undo(st); }
        replicas[i] = r;
        r->stats = root->stats;
        hipError_t e = hipSuccess;
        if (devices[i] != root->device) {
            int can = 0;
            e = hipDeviceCanAccessPeer(&can, devices[i], root->device);
            if (e == hipSuccess && can) {
                e = hipDeviceEnablePeerAccess(root->device, 0);       // direct xGMI reads; already-enabled is fine
                if (e != hipSuccess) { (void)hipGetLastError(); e = hipSuccess; }
            }
        }
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&streams[i], hipStreamNonBlocking);
        // all destinations' copies are queued before any is waited for: the root streams to its peers in parallel
        // (xGMI is point to point: one link per destination)
        if (e == hipSuccess && pb) e = hipMemcpyPeerAsync(r->d_points, devices[i], root->d_points, root->device, pb, streams[i]);
        if (e == hipSuccess && zb) e = hipMemcpyPeerAsync(r->d_zero, devices[i], root->d_zero, root->device, zb, streams[i]);
        if (e == hipSuccess && ub) e = hipMemcpyPeerAsync(r->d_upper, devices[i], root->d_upper, root->device, ub, streams[i]);
        if (e != hipSuccess) {
            fail(IDIST_ERR_HIP, "replicate to device %d: %s", devices[i], hipGetErrorString(e));
            drop_streams();
            return undo(IDIST_ERR_HIP);
        }
    }
    for (uint32_t i = 0; i < n_devices; i++) {
        hipSetDevice(devices[i]);
        hipError_t e = hipStreamSynchronize(streams[i]);
        if (e != hipSuccess) {
            fail(IDIST_ERR_HIP, "replicate to device %d: %s", devices[i], hipGetErrorString(e));
            drop_streams();
            return undo(IDIST_ERR_HIP);
        }
    }
    drop_streams();
    hipSetDevice(root->device);
    return IDIST_OK;
}

// ---- the same replication as RCCL broadcasts (one process, one communicator over the devices involved) ----
#ifndef IDIST_EMU
#include <dlfcn.h>
namespace {
// the six RCCL entry points this file needs, resolved on first use: libidist.so carries no link-time dependency on
// librccl (a process that never replicates never loads it; a process that already holds one — torch's — shares it)
struct Rccl {
    typedef void* comm_t;
    int (*CommInitAll)(comm_t*, int, const int*) = nullptr;
    int (*CommDestroy)(comm_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Broadcast)(const void*, void*, size_t, int, int, comm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool ok = false;
    std::string why;
    Rccl() {
        void* h = nullptr;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
            if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
        if (!h) { why = std::string("librccl.so not found: ") + (dlerror() ? dlerror() : "?"); return; }
        auto sym = [&](const char* n) { void* p = dlsym(h, n); if (!p && why.empty()) why = std::string("librccl: no symbol ") + n; return p; };
        CommInitAll = (int (*)(comm_t*, int, const int*))sym("ncclCommInitAll");
        CommDestroy = (int (*)(comm_t))sym("ncclCommDestroy");
        GroupStart = (int (*)())sym("ncclGroupStart");
        GroupEnd = (int (*)())sym("ncclGroupEnd");
        Broadcast = (int (*)(const void*, void*, size_t, int, int, comm_t, hipStream_t))sym("ncclBroadcast");
        GetErrorString = (const char* (*)(int))sym("ncclGetErrorString");
        ok = why.empty();
    }
    static Rccl& get() { static Rccl r; return r; }
};
constexpr int kNcclUint8 = 1;   // ncclDataType_t::ncclUint8 (rccl.h)
}  // namespace
#endif

idist_status idist_replicate_rccl(const idist_index* root, const int32_t* devices, uint32_t n_devices, idist_index** replicas,
                                  double* seconds) {
    if (!root || !replicas || (n_devices && !devices)) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    if (seconds) *seconds = 0.0;
#ifdef IDIST_EMU
    return idist_replicate(root, devices, n_devices, replicas);       // (the CPU emulator of tests/simt has no RCCL: same result)
#else
    for (uint32_t i = 0; i < n_devices; i++) replicas[i] = nullptr;
    if (n_devices == 0) return IDIST_OK;
    Rccl& R = Rccl::get();
    if (!R.ok) return fail(IDIST_ERR_UNSUPPORTED, "idist_replicate_rccl: %s", R.why.c_str());
    // ranks: the root's device first, then every other distinct destination device
    std::vector<int> devs{root->device};
    for (uint32_t i = 0; i < n_devices; i++)
        if (std::find(devs.begin(), devs.end(), (int)devices[i]) == devs.end()) devs.push_back((int)devices[i]);
    const int nr = (int)devs.size();
    std::vector<Rccl::comm_t> comms(nr, nullptr);
    std::vector<hipStream_t> streams(nr, nullptr);
    std::vector<int> first(nr, -1);                                   // the replica each rank receives into
    auto cleanup = [&](idist_status s) {
        const std::string keep = g_err;
        for (int r = 0; r < nr; r++) {
            if (streams[r]) { hipSetDevice(devs[r]); hipStreamDestroy(streams[r]); }
            if (comms[r]) R.CommDestroy(comms[r]);
        }
        if (s != IDIST_OK)
            for (uint32_t i = 0; i < n_devices; i++) { idist_index_free(replicas[i]); replicas[i] = nullptr; }
        hipSetDevice(root->device);
        g_err = keep;
        return s;
    };
    // nothing may still be writing the root's buffers (a build on another stream)
    if (hipSetDevice(root->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return fail(IDIST_ERR_HIP, "replicate: root device %d: %s", root->device, hipGetErrorString(hipGetLastError()));
    for (uint32_t i = 0; i < n_devices; i++) {
        idist_index* r = nullptr;
        const idist_status st = index_alloc(root->n, root->dim, &root->cfg, root->layer_len, root->n_upper, devices[i], &r);
        if (st != IDIST_OK) return cleanup(st);
        replicas[i] = r;
        r->stats = root->stats;
        const int rk = (int)(std::find(devs.begin(), devs.end(), (int)devices[i]) - devs.begin());
        if (first[rk] < 0) first[rk] = (int)i;
    }
    int rc = R.CommInitAll(comms.data(), nr, devs.data());
    if (rc != 0) return cleanup(fail(IDIST_ERR_HIP, "ncclCommInitAll over %d devices: %s", nr, R.GetErrorString(rc)));
    for (int r = 0; r < nr; r++)
        if (hipSetDevice(devs[r]) != hipSuccess || hipStreamCreateWithFlags(&streams[r], hipStreamNonBlocking) != hipSuccess)
            return cleanup(fail(IDIST_ERR_HIP, "replicate: stream on device %d: %s", devs[r], hipGetErrorString(hipGetLastError())));
    const size_t pb = (size_t)root->n * root->L.stride * 4, zb = (size_t)root->n * IDIST_M2 * 4, ub = root->upper_rows * IDIST_M * 4;
    struct Buf { const void* src; size_t bytes; int which; };
    const Buf bufs[3] = {{root->d_points, pb, 0}, {root->d_zero, zb, 1}, {root->d_upper, ub, 2}};
    auto dst_of = [&](const idist_index* x, int which) -> void* {
        return which == 0 ? (void*)x->d_points : (which == 1 ? (void*)x->d_zero : (void*)x->d_upper);
    };
    const auto t0 = std::chrono::steady_clock::now();
    for (const Buf& b : bufs) {
        if (!b.bytes) continue;
        if ((rc = R.GroupStart()) != 0) return cleanup(fail(IDIST_ERR_HIP, "ncclGroupStart: %s", R.GetErrorString(rc)));
        for (int r = 0; r < nr && rc == 0; r++) {
            // rank 0 = the root: it sends its own buffer and, if a replica lives on its device, receives into that one
            void* recv = first[r] >= 0 ? dst_of(replicas[first[r]], b.which) : (void*)b.src;
            rc = R.Broadcast(b.src, recv, b.bytes, kNcclUint8, 0, comms[r], streams[r]);   // (sendbuff is read on the root only)
        }
        const int rc2 = R.GroupEnd();
        if (rc != 0 || rc2 != 0) return cleanup(fail(IDIST_ERR_HIP, "ncclBroadcast: %s", R.GetErrorString(rc ? rc : rc2)));
    }
    for (int r = 0; r < nr; r++)
        if (hipSetDevice(devs[r]) != hipSuccess || hipStreamSynchronize(streams[r]) != hipSuccess)
            return cleanup(fail(IDIST_ERR_HIP, "replicate: broadcast to device %d: %s", devs[r], hipGetErrorString(hipGetLastError())));
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    // further replicas on a device that already holds one: plain device-to-device copies
    for (uint32_t i = 0; i < n_devices; i++) {
        const int rk = (int)(std::find(devs.begin(), devs.end(), (int)devices[i]) - devs.begin());
        if (first[rk] == (int)i) continue;
        hipSetDevice(devices[i]);
        for (const Buf& b : bufs)
            if (b.bytes && hipMemcpy(dst_of(replicas[i], b.which), dst_of(replicas[first[rk]], b.which), b.bytes, hipMemcpyDeviceToDevice) != hipSuccess)
                return cleanup(fail(IDIST_ERR_HIP, "replicate: copy on device %d: %s", devices[i], hipGetErrorString(hipGetLastError())));
    }
    return cleanup(IDIST_OK);
#endif
}

extern "C++" {
namespace {
// Calls that block on the host side by side (shards, the parts of a partitioned index): work(i) for every i < n with runs(i).  The
// first runs on the calling thread, every other on a thread of its own — or here, after the others were started, when no thread is
// to be had.  Every thread is joined before this returns.  True when one failed: *f is the first such i, with its status and
// message (g_err is thread-local: a worker's message is kept where it ran).
struct Failure { size_t i = 0; idist_status status = IDIST_OK; std::string msg; };
template <typename Runs, typename Work> bool fan_out(size_t n, Runs&& runs, Work&& work, Failure* f) {
    std::vector<idist_status> st(n, IDIST_OK);
    std::vector<std::string> msg(n);
    auto one = [&](size_t i) {
        st[i] = work(i);
        if (st[i] != IDIST_OK) msg[i] = g_err;
    };
    {
        std::vector<std::thread> threads;
        size_t first = n;
        for (size_t i = 0; i < n; i++) {
            if (!runs(i)) continue;
            if (first == n) { first = i; continue; }
            try {
                threads.emplace_back(one, i);
            } catch (...) {
                one(i);
            }
        }
        if (first < n) one(first);
        for (auto& t : threads) t.join();
    }
    for (size_t i = 0; i < n; i++)
        if (st[i] != IDIST_OK) { *f = Failure{i, st[i], msg[i]}; return true; }
    return false;
}
}  // namespace
}  // extern "C++"

idist_status idist_search_batch_sharded(const idist_index* const* replicas, idist_search_ctx* const* ctxs, uint32_t n_shards,
                                        const float* queries, uint32_t nq, uint32_t* out_pid, float* out_dist,
                                        uint32_t* out_count, uint32_t* out_counters) {
    if (!replicas || !ctxs || n_shards == 0) return fail(IDIST_ERR_INVALID_ARG, "no shards");
    for (uint32_t i = 0; i < n_shards; i++) {
        CHK(check_ctx(replicas[i], ctxs[i]));
        if (replicas[i]->n != replicas[0]->n || replicas[i]->dim != replicas[0]->dim ||
            replicas[i]->cfg.ef_search != replicas[0]->cfg.ef_search)
            return fail(IDIST_ERR_INVALID_ARG, "shard %u is not a replica of shard 0 (n, dim or ef_search differ)", i);
        for (uint32_t j = 0; j < i; j++)
            if (ctxs[j] == ctxs[i]) return fail(IDIST_ERR_INVALID_ARG, "shards %u and %u share a search context", j, i);
    }
    if (nq == 0) return IDIST_OK;
    if (!queries || !out_count) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    const uint32_t ef = replicas[0]->cfg.ef_search, dim = replicas[0]->dim;
    // contiguous block partition, the reference's own concurrency model (callers split queries over threads)
    auto lo_of = [&](size_t i) { return (uint32_t)((uint64_t)nq * i / n_shards); };
    auto shard = [&](size_t i) {
        const uint32_t lo = lo_of(i), hi = lo_of(i + 1);
        return idist_search_batch(replicas[i], ctxs[i], queries + (size_t)lo * dim, hi - lo,
                                  out_pid ? out_pid + (size_t)lo * ef : nullptr, out_dist ? out_dist + (size_t)lo * ef : nullptr,
                                  out_count + lo, out_counters ? out_counters + (size_t)lo * 3 : nullptr);
    };
    Failure f;
    if (fan_out(n_shards, [&](size_t i) { return lo_of(i + 1) != lo_of(i); }, shard, &f))
        return fail(f.status, "shard %u (device %d): %s", (uint32_t)f.i, replicas[f.i]->device, f.msg.c_str());
    return IDIST_OK;
}

// ---- partitioned index: several indexes searched as one, merged on the device ----
static idist_status launch_merge(MergeArgs a, hipStream_t stream) {
    const size_t keys = (size_t)a.n_lists * a.width * 8;
    const bool lds = keys + kMergeHeadBytes <= kMergeLdsBudget;
    a.vec4 = (a.width % 4u == 0u && ((uintptr_t)a.pid % 16u) == 0 && ((uintptr_t)a.dist % 16u) == 0) ? 1u : 0u;
    const uint32_t grid = std::min<uint32_t>(a.nq, 16384u);          // one wave per query; the kernel strides over the rest
    if (lds) {
        auto kM = merge_topk_kernel<true>;
        IDIST_LAUNCH(kM, grid, 64, kMergeHeadBytes + keys, stream, a);
    } else {
        auto kM = merge_topk_kernel<false>;
        IDIST_LAUNCH(kM, grid, 64, (size_t)kMergeHeadBytes, stream, a);
    }
    HIPCHK(hipGetLastError());
    return IDIST_OK;
}

idist_status idist_merge_topk_device(const void* d_pid, const void* d_dist, const void* d_count, const void* d_counters,
                                     uint32_t n_lists, uint32_t nq, uint32_t width, const uint32_t* base, uint32_t out_width,
                                     void* d_out_pid, void* d_out_dist, void* d_out_count, void* d_out_counters,
                                     int32_t device, void* hip_stream) {
    const uint32_t max_w = IDIST_MAX_EF;
    if (n_lists == 0 || n_lists > kMergeMaxLists) return fail(IDIST_ERR_INVALID_ARG, "n_lists %u out of [1,%u]", n_lists, kMergeMaxLists);
    if (width == 0 || width > max_w || out_width == 0 || out_width > max_w)
        return fail(IDIST_ERR_INVALID_ARG, "width %u / out_width %u out of [1,%u]", width, out_width, max_w);
    if (!base) return fail(IDIST_ERR_INVALID_ARG, "base is null");
    if (nq == 0) return IDIST_OK;
    if (!d_pid || !d_dist || !d_count || !d_out_pid || !d_out_dist || !d_out_count) return fail(IDIST_ERR_INVALID_ARG, "null device pointer");
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) return fail(IDIST_ERR_NO_DEVICE, "no HIP device visible; libidist has no CPU path");
    if (device < 0 || device >= cnt) return fail(IDIST_ERR_INVALID_ARG, "device %d out of range [0,%d)", device, cnt);
    HIPCHK(hipSetDevice(device));
    MergeArgs a{};
    a.pid = (const uint32_t*)d_pid; a.dist = (const uint32_t*)d_dist; a.count = (const uint32_t*)d_count;
    a.counters = (const uint32_t*)d_counters;
    a.n_lists = n_lists; a.nq = nq; a.width = width; a.out_width = out_width;
    a.out_pid = (uint32_t*)d_out_pid; a.out_dist = (uint32_t*)d_out_dist; a.out_count = (uint32_t*)d_out_count;
    a.out_counters = d_counters ? (uint32_t*)d_out_counters : nullptr;
    for (uint32_t l = 0; l < n_lists; l++) a.base[l] = base[l];
    return launch_merge(a, (hipStream_t)hip_stream);
}

// dim / metric / ef_search of every part against part 0, and the id space; fills base[] (idist_index_set_ef_search can change a
// part at any time, so this runs at every call)
static idist_status partitioned_check(idist_partitioned* p, uint32_t* ef_out) {
    const idist_index* first = p->parts[0].idx;
    uint64_t n = 0;
    for (size_t i = 0; i < p->parts.size(); i++) {
        const idist_index* ix = p->parts[i].idx;
        if (ix->uid != p->parts[i].uid) return fail(IDIST_ERR_INVALID_ARG, "part %zu is not the index this object was made for", i);
        if (ix->dim != first->dim) return fail(IDIST_ERR_INVALID_ARG, "part %zu: dim %u differs from part 0's %u", i, ix->dim, first->dim);
        if (ix->cfg.metric != first->cfg.metric) return fail(IDIST_ERR_INVALID_ARG, "part %zu: metric %d differs from part 0's %d", i, ix->cfg.metric, first->cfg.metric);
        if (ix->cfg.ef_search != first->cfg.ef_search)
            return fail(IDIST_ERR_INVALID_ARG, "part %zu: ef_search %u differs from part 0's %u", i, ix->cfg.ef_search, first->cfg.ef_search);
        // DOT: one query augmentation and one report serve all parts, so every part must have been made with the same S, bit for bit
        if (is_dot(ix->cfg) && memcmp(&ix->dot_S, &first->dot_S, 4) != 0)
            return fail(IDIST_ERR_INVALID_ARG, "part %zu: dot_bound %.9g differs from part 0's %.9g (build every part with the bound of the whole set)",
                        i, (double)ix->dot_S, (double)first->dot_S);
        p->base[i] = (uint32_t)n;
        n += ix->n;
        if (n >= (uint64_t)kInvalid) return fail(IDIST_ERR_INVALID_ARG, "part %zu: %llu points together do not fit a PointId", i, (unsigned long long)n);
    }
    p->base[p->parts.size()] = (uint32_t)n;
    if (ef_out) *ef_out = first->cfg.ef_search;
    return IDIST_OK;
}

idist_status idist_partitioned_new(const idist_index* const* parts, uint32_t n_parts, idist_partitioned** out) {
    if (!out) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (n_parts == 0 || n_parts > kMergeMaxLists) return fail(IDIST_ERR_INVALID_ARG, "n_parts %u out of [1,%u]", n_parts, kMergeMaxLists);
    if (!parts) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    for (uint32_t i = 0; i < n_parts; i++)
        if (!parts[i]) return fail(IDIST_ERR_INVALID_ARG, "part %u is null", i);
    idist_partitioned* p = new idist_partitioned();
    p->uid = fresh_uid();
    auto bail = [&](idist_status s) {
        const std::string keep = g_err;
        idist_partitioned_free(p);
        g_err = keep;
        return s;
    };
    p->parts.resize(n_parts);
    for (uint32_t i = 0; i < n_parts; i++) { p->parts[i].idx = parts[i]; p->parts[i].uid = parts[i]->uid; }
    p->dim = parts[0]->dim;
    p->metric = parts[0]->cfg.metric;
    p->merge_device = parts[0]->device;
    p->dot_S = parts[0]->dot_S;
    idist_status s = partitioned_check(p, nullptr);
    if (s != IDIST_OK) return bail(s);
    for (uint32_t i = 0; i < n_parts; i++) {
        idist_partitioned::Part& pt = p->parts[i];
        int slot = -1;
        for (size_t d = 0; d < p->devs.size(); d++) if (p->devs[d].device == parts[i]->device) slot = (int)d;
        if (slot < 0) {
            p->devs.emplace_back();
            p->devs.back().device = parts[i]->device;
            slot = (int)p->devs.size() - 1;
        }
        pt.dev_slot = slot;
        if (parts[i]->n && (s = idist_search_ctx_new(parts[i], 0, &pt.ctx)) != IDIST_OK) return bail(s);
    }
    hipError_t e;
    if ((e = hipSetDevice(p->merge_device)) != hipSuccess || (e = hipStreamCreate(&p->stream)) != hipSuccess ||
        (e = hipEventCreate(&p->ev0)) != hipSuccess || (e = hipEventCreate(&p->ev1)) != hipSuccess)
        return bail(fail(IDIST_ERR_HIP, "partitioned index set-up failed: %s", hipGetErrorString(e)));
    *out = p;
    return IDIST_OK;
}

void idist_partitioned_free(idist_partitioned* p) {
    if (!p) return;
    // (the parts are borrowed and may already be gone: nothing of them is touched here)
    for (auto& pt : p->parts) idist_search_ctx_free(pt.ctx);
    if (p->ev0) hipEventDestroy(p->ev0);
    if (p->ev1) hipEventDestroy(p->ev1);
    if (p->stream) hipStreamDestroy(p->stream);
    delete p;                      // (the staging of the object, its parts and devices: as in idist_search_ctx_free)
}

idist_status idist_partitioned_get_info(const idist_partitioned* p, idist_partitioned_info* out) {
    if (!p || !out) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    memset(out, 0, sizeof(*out));
    uint32_t ef = 0;
    CHK(partitioned_check(const_cast<idist_partitioned*>(p), &ef));
    out->n_parts = (uint32_t)p->parts.size();
    out->dim = p->dim;
    out->ef_search = ef;
    out->metric = p->metric;
    out->merge_device = p->merge_device;
    out->n = p->base[p->parts.size()];
    for (size_t i = 0; i <= p->parts.size(); i++) out->base[i] = p->base[i];
    return IDIST_OK;
}

// staging on the merge device for P lists of `width` per query and a result of `out_width` (the merge device is current)
static idist_status partitioned_reserve(idist_partitioned* p, uint32_t nq, uint32_t width, uint32_t out_width) {
    const size_t P = p->parts.size(), slab = P * nq * width, o = (size_t)nq * out_width;
    CHK(p->s_pid.grow(slab * 4));
    CHK(p->s_dist.grow(slab * 4));
    CHK(p->s_cnt.grow(P * nq * 4));
    CHK(p->s_ctr.grow(P * nq * 12));
    CHK(p->o_cnt.grow((size_t)nq * 4));
    CHK(p->o_ctr.grow((size_t)nq * 12));
    CHK(p->o_pid.grow(o * 4));
    CHK(p->o_dist.grow(o * 4));
    return IDIST_OK;
}

static idist_status bruteforce_impl(const idist_index* idx, const float* queries, uint32_t nq, uint32_t k, uint32_t* out_pid,
                                    float* out_dist, bool raw);

// What the report behind the merge needs of the batch's queries — s(q), for a metric that has one — on the merge device (which is
// current); enqueued on p->stream
static idist_status partitioned_prepare_report(idist_partitioned* p, const float* queries, uint32_t nq) {
    const MetricPasses metric(p);
    if (!metric.sq_floats(nq)) return IDIST_OK;
    const size_t qb = (size_t)nq * p->dim * 4;
    CHK(p->d_qm.grow(qb));
    CHK(p->d_sq.grow(metric.sq_floats(nq) * 4));
    HIPCHK(hipMemcpyAsync(p->d_qm, queries, qb, hipMemcpyHostToDevice, p->stream));
    return metric.prepare(p->d_qm, nullptr, p->d_sq, nq, p->stream, nullptr);
}

// the merge kernel between two events + its result to the host; every part's list is complete in the staging memory.  The parts
// hand in the index's raw squared-L2 distances: the metric's report runs HERE, after the merge (partitioned_prepare_report ran on
// this stream before) — the merge relies on every list being strictly ordered by (distance bits, id) with non-negative keys, which
// halving can break for denormal distances.
static idist_status partitioned_merge(idist_partitioned* p, uint32_t nq, uint32_t width, uint32_t out_width, bool counters,
                                      uint32_t* out_pid, float* out_dist, uint32_t* out_count, uint32_t* out_counters) {
    MergeArgs a{};
    a.pid = p->s_pid; a.dist = (const uint32_t*)p->s_dist.p; a.count = p->s_cnt; a.counters = counters ? p->s_ctr.p : nullptr;
    a.n_lists = (uint32_t)p->parts.size(); a.nq = nq; a.width = width; a.out_width = out_width;
    a.out_pid = p->o_pid; a.out_dist = (uint32_t*)p->o_dist.p; a.out_count = p->o_cnt; a.out_counters = counters ? p->o_ctr.p : nullptr;
    for (uint32_t l = 0; l < a.n_lists; l++) a.base[l] = p->base[l];
    HIPCHK(hipEventRecord(p->ev0, p->stream));
    CHK(launch_merge(a, p->stream));
    HIPCHK(hipEventRecord(p->ev1, p->stream));
    p->timed = true;
    CHK(MetricPasses(p).report(p->o_dist, p->d_sq, nq, out_width, p->stream));
    const size_t ob = (size_t)nq * out_width * 4;
    HIPCHK(hipMemcpyAsync(out_pid, p->o_pid, ob, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipMemcpyAsync(out_dist, p->o_dist, ob, hipMemcpyDeviceToHost, p->stream));
    if (out_count) HIPCHK(hipMemcpyAsync(out_count, p->o_cnt, (size_t)nq * 4, hipMemcpyDeviceToHost, p->stream));
    if (counters) HIPCHK(hipMemcpyAsync(out_counters, p->o_ctr, (size_t)nq * 12, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    return IDIST_OK;
}

// ---- the steps the partitioned calls share ----
static int32_t part_device(const idist_partitioned* p, size_t i) { return p->devs[p->parts[i].dev_slot].device; }

// a part's failure as the caller sees it (msg by value: it may be g_err itself, which fail() writes)
static idist_status part_failed(const idist_partitioned* p, size_t i, idist_status s, std::string msg) {
    return fail(s, "part %zu (device %d): %s", i, part_device(p, i), msg.c_str());
}

extern "C++" {
namespace {
// part(i) for every non-empty part, side by side (fan_out); the first failure comes back as the part's
template <typename Work> idist_status partitioned_fan_out(idist_partitioned* p, Work&& part) {
    Failure f;
    if (fan_out(p->parts.size(), [&](size_t i) { return p->parts[i].ctx != nullptr; }, part, &f)) return part_failed(p, f.i, f.status, f.msg);
    return IDIST_OK;
}

// fn(dv) for every device that has something to search, with that device current (it stays current)
template <typename Fn> idist_status for_each_used_device(idist_partitioned* p, Fn&& fn) {
    for (size_t d = 0; d < p->devs.size(); d++) {
        bool used = false;
        for (auto& pt : p->parts) used |= pt.ctx && pt.dev_slot == (int)d;
        if (!used) continue;
        HIPCHK(hipSetDevice(p->devs[d].device));
        CHK(fn(p->devs[d]));
    }
    return IDIST_OK;
}
}  // namespace
}  // extern "C++"

// The batch's queries, once per distinct device that has something to search, as the parts' launches read them (prepared = true):
// Dev::d_q holds the [nq][kdim] rows in front (a metric whose prepare cannot run in place: followed by the queries as uploaded).
// Leaves another device current.  with_sq: a metric with a report term also leaves s(q) in Dev::d_sq (the range search's limits).
static idist_status partitioned_upload_queries(idist_partitioned* p, const float* queries, uint32_t nq, bool with_sq = false) {
    const MetricPasses metric(p);
    const size_t qb = (size_t)nq * p->dim * 4, qa = metric.in_place() ? 0 : metric.qk_floats(nq) * 4;
    return for_each_used_device(p, [&](idist_partitioned::Dev& dv) -> idist_status {
        CHK(dv.d_q.grow(qa + qb));
        HIPCHK(hipMemcpy(dv.d_q + qa / 4, queries, qb, hipMemcpyHostToDevice));
        const bool sq = with_sq && metric.sq_floats(nq) != 0;
        if (sq) CHK(dv.d_sq.grow(metric.sq_floats(nq) * 4));
        if (metric.any()) {                              // prepared once per device; the parts' launches take them as they are
            CHK(metric.prepare(dv.d_q + qa / 4, dv.d_q, sq ? dv.d_sq.p : nullptr, nq, nullptr, nullptr));
            HIPCHK(hipStreamSynchronize(nullptr));
        }
        return IDIST_OK;
    });
}

// A part away from the merge device: its (pid, dist, count[, rung][, counters]) arrays, [nq] rows of `width`, to slice i of the
// staging memory on the merge device, one peer copy per array on the part's stream (the part's device is current)
static idist_status partitioned_send(idist_partitioned* p, size_t i, uint32_t nq, uint32_t width, const uint32_t* pid, const void* dist,
                                     const uint32_t* cnt, const uint32_t* rung, const uint32_t* ctr) {
    const int32_t dev = part_device(p, i), to = p->merge_device;
    hipStream_t stream = p->parts[i].ctx->stream;
    const size_t row = (size_t)nq * width;
    HIPCHK(hipMemcpyPeerAsync(p->s_pid + i * row, to, pid, dev, row * 4, stream));
    HIPCHK(hipMemcpyPeerAsync(p->s_dist + i * row, to, dist, dev, row * 4, stream));
    HIPCHK(hipMemcpyPeerAsync(p->s_cnt + i * nq, to, cnt, dev, (size_t)nq * 4, stream));
    if (rung) HIPCHK(hipMemcpyPeerAsync(p->s_rung + i * nq, to, rung, dev, (size_t)nq * 4, stream));
    if (ctr) HIPCHK(hipMemcpyPeerAsync(p->s_ctr + i * nq * 3, to, ctr, dev, (size_t)nq * 12, stream));
    return IDIST_OK;
}

// an empty part hands in lists of length 0 and has done no work: its counts and counters in the staging memory, on p->stream (the
// merge device is current)
static idist_status partitioned_zero_empty_parts(idist_partitioned* p, uint32_t nq, bool counters) {
    for (size_t i = 0; i < p->parts.size(); i++) {
        if (p->parts[i].ctx) continue;
        HIPCHK(hipMemsetAsync(p->s_cnt + i * nq, 0, (size_t)nq * 4, p->stream));
        if (counters) HIPCHK(hipMemsetAsync(p->s_ctr + i * nq * 3, 0, (size_t)nq * 12, p->stream));
    }
    return IDIST_OK;
}

// the parts' rungs [P][nq] as the caller has them, [nq][P]; an empty part's column keeps the IDIST_RUNG_NONE written up front
static void partitioned_transpose_rungs(const idist_partitioned* p, const std::vector<uint32_t>& rungs, uint32_t nq, uint32_t* out_rung) {
    const size_t P = p->parts.size();
    for (size_t i = 0; out_rung && i < P; i++) {
        if (!p->parts[i].ctx) continue;
        for (uint32_t q = 0; q < nq; q++) out_rung[(size_t)q * P + i] = rungs[i * nq + q];
    }
}

idist_status idist_partitioned_search_batch(idist_partitioned* p, const float* queries, uint32_t nq, uint32_t* out_pid,
                                            float* out_dist, uint32_t* out_count, uint32_t* out_counters) {
    if (!p) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    uint32_t ef = 0;
    CHK(partitioned_check(p, &ef));
    if (nq == 0) return IDIST_OK;
    if (!queries || !out_count) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    const size_t P = p->parts.size();
    if (p->base[P] == 0 || ef == 0) {                    // core/lib.rs:359-361
        memset(out_count, 0, (size_t)nq * 4);
        if (out_counters) memset(out_counters, 0, (size_t)nq * 12);
        return IDIST_OK;
    }
    if (!out_pid || !out_dist) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    const bool counters = out_counters != nullptr;
    const size_t row = (size_t)nq * ef;
    HIPCHK(hipSetDevice(p->merge_device));
    CHK(partitioned_reserve(p, nq, ef, ef));
    CHK(partitioned_prepare_report(p, queries, nq));
    // 1. the queries, once per distinct device that has something to search
    CHK(partitioned_upload_queries(p, queries, nq));
    // 2. every part on its own stream: on the merge device straight into its slice of the staging memory, elsewhere into memory of
    //    its own device followed by one peer copy per array
    auto enqueue = [&](size_t i) -> idist_status {
        idist_partitioned::Part& pt = p->parts[i];
        const int32_t dev = p->devs[pt.dev_slot].device;
        uint32_t *s_pid = p->s_pid + i * row, *s_cnt = p->s_cnt + i * nq, *s_ctr = p->s_ctr + i * nq * 3;
        float* s_dist = p->s_dist + i * row;
        HIPCHK(hipSetDevice(dev));
        if (dev == p->merge_device)
            return search_batch_device_impl(pt.idx, pt.ctx, p->devs[pt.dev_slot].d_q, nq, s_pid, s_dist, s_cnt, counters ? s_ctr : nullptr, pt.ctx->stream, true);
        CHK(pt.r_pid.grow(row * 4));
        CHK(pt.r_dist.grow(row * 4));
        CHK(pt.r_cnt.grow((size_t)nq * 4));
        CHK(pt.r_ctr.grow((size_t)nq * 12));
        uint32_t* r_ctr = counters ? pt.r_ctr.p : nullptr;
        CHK(search_batch_device_impl(pt.idx, pt.ctx, p->devs[pt.dev_slot].d_q, nq, pt.r_pid, pt.r_dist, pt.r_cnt, r_ctr, pt.ctx->stream, true));
        return partitioned_send(p, i, nq, ef, pt.r_pid, pt.r_dist, pt.r_cnt, nullptr, r_ctr);
    };
    for (size_t i = 0; i < P; i++)
        if (p->parts[i].ctx) CHK(enqueue(i));
    HIPCHK(hipSetDevice(p->merge_device));
    CHK(partitioned_zero_empty_parts(p, nq, counters));
    // 3. wait for every part and read its device-side status.  Strict ties: a part whose tie region overflowed now has the larger
    //    region (or the HBM bags) and is searched again — for as long as the escalation makes progress, the bound idist_search_batch
    //    puts on its own loop; the merge never sees a list from an overflowed launch
    for (size_t i = 0; i < P; i++) {
        idist_partitioned::Part& pt = p->parts[i];
        if (!pt.ctx) continue;
        for (;;) {
            HIPCHK(hipSetDevice(p->devs[pt.dev_slot].device));
            HIPCHK(hipStreamSynchronize(pt.ctx->stream));
            idist_status s;
            if (status_asks_retry(pt.idx, pt.ctx, &s)) {
                CHK(enqueue(i));
                continue;
            }
            if (s == IDIST_OK) break;
            return part_failed(p, i, s, g_err);
        }
    }
    // 4. the union
    HIPCHK(hipSetDevice(p->merge_device));
    return partitioned_merge(p, nq, ef, ef, counters, out_pid, out_dist, out_count, out_counters);
}

idist_status idist_partitioned_bruteforce(idist_partitioned* p, const float* queries, uint32_t nq, uint32_t k,
                                          uint32_t* out_pid, float* out_dist) {
    if (!p) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    CHK(partitioned_check(p, nullptr));
    if (nq == 0) return IDIST_OK;
    if (k == 0 || k > IDIST_MAX_EF) return fail(IDIST_ERR_INVALID_ARG, "k %u out of [1,%u]", k, IDIST_MAX_EF);
    if (!queries || !out_pid || !out_dist) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    const size_t P = p->parts.size(), row = (size_t)nq * k;
    HIPCHK(hipSetDevice(p->merge_device));
    CHK(partitioned_reserve(p, nq, k, k));
    CHK(partitioned_prepare_report(p, queries, nq));
    std::vector<uint32_t> h_pid(row), h_cnt(nq);
    std::vector<float> h_dist(row);
    for (size_t i = 0; i < P; i++) {
        const idist_index* ix = p->parts[i].idx;
        const uint32_t kp = std::min(k, ix->n);                   // what this part contributes per query
        if (kp) {
            const idist_status s = bruteforce_impl(ix, queries, nq, kp, h_pid.data(), h_dist.data(), true);
            if (s != IDIST_OK) return part_failed(p, i, s, g_err);
            HIPCHK(hipSetDevice(p->merge_device));
            HIPCHK(hipMemcpy2D(p->s_pid + i * row, (size_t)k * 4, h_pid.data(), (size_t)kp * 4, (size_t)kp * 4, nq, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy2D(p->s_dist + i * row, (size_t)k * 4, h_dist.data(), (size_t)kp * 4, (size_t)kp * 4, nq, hipMemcpyHostToDevice));
        }
        std::fill(h_cnt.begin(), h_cnt.end(), kp);
        HIPCHK(hipMemcpy(p->s_cnt + i * nq, h_cnt.data(), (size_t)nq * 4, hipMemcpyHostToDevice));
    }
    return partitioned_merge(p, nq, k, k, false, out_pid, out_dist, nullptr, nullptr);
}

idist_status idist_partitioned_last_search_kernel_ms(idist_partitioned* p, float* ms, uint32_t cap, uint32_t* n_out) {
    if (!p || !ms || !n_out) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    const uint32_t take = (uint32_t)std::min<size_t>(p->parts.size(), cap);
    for (uint32_t i = 0; i < take; i++) {
        idist_search_ctx* c = p->parts[i].ctx;
        ms[i] = c ? -1.0f : 0.0f;                                    // empty part: no kernel; no timed launch (yet): -1
        if (c && c->n_rec) CHK(resolve_time(c, c->recs[(c->n_rec - 1) % IDIST_EVENT_RING], &ms[i]));
    }
    *n_out = take;
    return IDIST_OK;
}

idist_status idist_partitioned_last_merge_ms(idist_partitioned* p, float* ms) {
    if (!p || !ms) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    if (!p->timed) return fail(IDIST_ERR_INVALID_ARG, "no merge kernel has run through this object yet");
    HIPCHK(hipEventSynchronize(p->ev1));
    HIPCHK(hipEventElapsedTime(ms, p->ev0, p->ev1));
    return IDIST_OK;
}

// idist_distance_batch (bound = false) and idist_filter_bound_batch (bound = true): one kernel over [nq][n_ids] (query, id) pairs
// between the metric's passes.  A bound stays a bound under both reports: half a lower bound is a lower bound of half, and DOT's
// report is non-decreasing — "no bound" (raw 0) becomes the trivial bound -t / 2 there.
static idist_status pairs_batch(const idist_index* idx, const float* queries, uint32_t nq, const uint32_t* ids, uint32_t n_ids,
                                float* out, bool bound) {
    if (!idx) return fail(IDIST_ERR_INVALID_ARG, "idx is null");
    if (nq == 0 || n_ids == 0) return IDIST_OK;
    if (!queries || !ids || !out) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    HIPCHK(hipSetDevice(idx->device));
    const MetricPasses metric(idx);
    const size_t qb = (size_t)nq * idx->dim * 4, ib = (size_t)nq * n_ids * 4;
    bool have_filter = false;
    if (bound) {
        if (filter_applies(idx)) CHK(filter_ensure(idx));
        have_filter = idx->filt_state.load(std::memory_order_acquire) == 1;
        if (!have_filter && metric.report_keeps_zero()) {                // no filter for this index: no bound
            memset(out, 0, ib);
            return IDIST_OK;
        }
    }
    Scratch mem;
    float *d_q = nullptr, *d_out = nullptr;
    uint32_t* d_ids = nullptr;
    CHK(mem.alloc(&d_q, qb / 4));
    CHK(mem.alloc(&d_out, ib / 4));
    CHK(mem.alloc(&d_ids, ib / 4));
    HIPCHK(hipMemcpy(d_q, queries, qb, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_ids, ids, ib, hipMemcpyHostToDevice));
    const float *d_qk = nullptr, *d_sq = nullptr;                        // what the kernel reads: [nq][kdim]
    CHK(metric.prepare_own(d_q, mem, nq, nullptr, &d_qk, &d_sq));
    const uint32_t chunks = (n_ids + 63u) / 64u;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((uint64_t)nq * chunks, 1u << 20);
    const size_t smem = smem_bytes(idx->L.stride, 0, false);
    IndexView view = idx->view();
    // the bound of the format wide searches of this index use
    int basis = idx->filt_format.load(std::memory_order_relaxed);
    if (const char* e = test_env("IDIST_FILTER_BASIS")) {               // (no context here: the knob as a new context would sample it)
        if (bound && have_filter) CHK(filter_basis_forced_check(idx, filter_basis_knob(e)));
        basis = filter_basis_knob(e) ? filter_basis_knob(e) : basis;
    }
    const bool principal = bound && have_filter && idx->filt_p.rows && basis == IDIST_FILTER_FORMAT_PRINCIPAL;
    if (principal) { view.f2 = view.f; view.f = idx->filt_p; }
#define LAUNCH_PAIRS(NB_, RS_, TAIL_)                                                                 \
    if (bound && principal) {                                                                         \
        launched = BoundLaunch<NB_, RS_, TAIL_, GeoKernels<NB_>::thin_search>::go(grid, smem, view, d_qk, nq, d_ids, n_ids, d_out); \
    } else if (bound) {                                                                               \
        auto kD = filter_bound_kernel<NB_, RS_, TAIL_>;                                               \
        IDIST_LAUNCH(kD, grid, 64, smem, (hipStream_t) nullptr, view, d_qk, nq, d_ids, n_ids, d_out); \
    } else {                                                                                          \
        auto kD = distance_batch_kernel<NB_, RS_, TAIL_>;                                             \
        IDIST_LAUNCH(kD, grid, 64, smem, (hipStream_t) nullptr, view, d_qk, nq, d_ids, n_ids, d_out); \
    }
    bool launched = true;
    if (have_filter || !bound) IDIST_DISPATCH(idx->L, LAUNCH_PAIRS);
    else HIPCHK(hipMemset(d_out, 0, ib));
#undef LAUNCH_PAIRS
    if (!launched) return fail(IDIST_ERR_INTERNAL, "no principal bound kernel for this row geometry (stride %u)", idx->L.stride);
    HIPCHK(hipGetLastError());
    CHK(metric.report(d_out, d_sq, nq, n_ids, nullptr));
    HIPCHK(hipMemcpy(out, d_out, ib, hipMemcpyDeviceToHost));
    return IDIST_OK;
}

idist_status idist_distance_batch(const idist_index* idx, const float* queries, uint32_t nq, const uint32_t* ids,
                                  uint32_t n_ids, float* out_dist) {
    return pairs_batch(idx, queries, nq, ids, n_ids, out_dist, false);
}

idist_status idist_filter_bound_batch(const idist_index* idx, const float* queries, uint32_t nq, const uint32_t* ids,
                                      uint32_t n_ids, float* out_bound) {
    return pairs_batch(idx, queries, nq, ids, n_ids, out_bound, true);
}

// raw (both brute-force paths): the queries are prepared, the squared-L2 distances of the index are left as they are — the
// partitioned brute force reports them after its merge
static idist_status bruteforce_scan(const idist_index* idx, const float* queries, uint32_t nq, uint32_t k,
                                    uint32_t* out_pid, float* out_dist, bool raw) {
    if (!idx) return fail(IDIST_ERR_INVALID_ARG, "idx is null");
    if (nq == 0) return IDIST_OK;
    if (k == 0 || k > IDIST_MAX_EF) return fail(IDIST_ERR_INVALID_ARG, "k %u out of [1,%u]", k, IDIST_MAX_EF);
    if (!queries || !out_pid || !out_dist) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    HIPCHK(hipSetDevice(idx->device));
    const MetricPasses metric(idx);
    const size_t qb = (size_t)nq * idx->dim * 4, ob = (size_t)nq * k * 4;
    Scratch mem;
    float *d_q = nullptr, *d_dist = nullptr;
    uint32_t *d_pid = nullptr, *d_next = nullptr;
    CHK(mem.alloc(&d_q, qb / 4));
    CHK(mem.alloc(&d_dist, ob / 4));
    CHK(mem.alloc(&d_pid, ob / 4));
    CHK(mem.alloc(&d_next, 64));
    HIPCHK(hipMemset(d_next, 0, 256));
    HIPCHK(hipMemcpy(d_q, queries, qb, hipMemcpyHostToDevice));
    const float *d_qk = nullptr, *d_sq = nullptr;                        // what the kernel reads: [nq][kdim]
    CHK(metric.prepare_own(d_q, mem, nq, nullptr, &d_qk, &d_sq));
    const uint32_t wcap = topk_wcap(k);
    const size_t smem = smem_bytes(idx->L.stride, wcap, false);
    const uint32_t grid = std::min<uint32_t>(nq, (uint32_t)idx->n_cu * 16);
    IndexView view = idx->view();
#define LAUNCH_BF(NB_, RS_, TAIL_)                                                                          \
    {                                                                                                       \
        auto kF = bruteforce_kernel<NB_, RS_, TAIL_>;                                                       \
        IDIST_LAUNCH(kF, grid, 64, smem, (hipStream_t) nullptr, view, d_qk, nq, k, wcap, d_pid, d_dist, d_next); \
    }
    IDIST_DISPATCH(idx->L, LAUNCH_BF);
#undef LAUNCH_BF
    HIPCHK(hipGetLastError());
    if (!raw) CHK(metric.report(d_dist, d_sq, nq, k, nullptr));
    HIPCHK(hipMemcpy(out_pid, d_pid, ob, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_dist, d_dist, ob, hipMemcpyDeviceToHost));
    return IDIST_OK;
}


// Wide-batch exact k-NN: f32-MFMA -2QP^T filter + canonical re-rank (idist_mfma.hpp).  Returns
// IDIST_ERR_INTERNAL with *fell_back = 1 if a candidate list overflowed (caller rescans).
static idist_status bruteforce_mfma(const idist_index* idx, const float* queries, uint32_t nq, uint32_t k,
                                    uint32_t* out_pid, float* out_dist, int* fell_back, bool raw) {
    *fell_back = 0;
    const MetricPasses metric(idx);
    const uint32_t n = idx->n, stride = idx->L.stride;
    uint32_t S = 32768;
    if (const char* e = test_env("IDIST_BF_SAMPLE")) S = (uint32_t)atoi(e);
    S = std::min(std::max(S, k), n);
    const uint32_t S_pad = (S + kTN - 1) / kTN * kTN;
    const uint32_t QC = 8192;                                    // queries per pass (bounds the dense sample matrix)
    const uint32_t cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((uint64_t)8 * k * n / S + 256, 1024), 1u << 16);
    Scratch mem;
    float *d_qnat = nullptr, *d_qb = nullptr, *d_qn = nullptr, *d_pn = nullptr, *d_dense = nullptr, *d_thr = nullptr, *d_dist = nullptr;
    float *d_qup = nullptr, *d_sq = nullptr;                     // where a pass's queries are uploaded, their s(q); d_qnat: [qc][kdim], what the kernels read
    uint32_t *d_cand = nullptr, *d_cnt = nullptr, *d_pid = nullptr, *d_ovf = nullptr;
    const uint32_t qc_max = std::min(nq, QC);
    const uint32_t qc_pad = (qc_max + kTM - 1) / kTM * kTM;
    CHK(mem.alloc(&d_qnat, (size_t)qc_max * idx->kdim));
    d_qup = d_qnat;
    if (!metric.in_place()) {                                    // (prepare widens the rows: the upload needs a buffer of its own)
        CHK(mem.alloc(&d_qup, (size_t)qc_max * idx->dim));
        CHK(mem.alloc(&d_sq, metric.sq_floats(qc_max)));
    }
    CHK(mem.alloc(&d_qb, (size_t)qc_pad * stride));
    CHK(mem.alloc(&d_qn, qc_pad));
    CHK(mem.alloc(&d_pn, n));
    CHK(mem.alloc(&d_dense, (size_t)qc_pad * S_pad));
    CHK(mem.alloc(&d_thr, qc_pad));
    CHK(mem.alloc(&d_cand, (size_t)qc_max * cap));
    CHK(mem.alloc(&d_cnt, qc_pad));
    CHK(mem.alloc(&d_pid, (size_t)qc_max * k));
    CHK(mem.alloc(&d_dist, (size_t)qc_max * k));
    CHK(mem.alloc(&d_ovf, 64));
    HIPCHK(hipMemset(d_ovf, 0, 256));
    hipStream_t st = nullptr;
    const uint32_t ngrid = std::min<uint32_t>(n, (uint32_t)idx->n_cu * 32);
    IDIST_LAUNCH(row_norms_kernel, ngrid, 64, 0, st, idx->d_points, n, stride, d_pn);
    std::vector<float> pn_h(n);
    HIPCHK(hipMemcpy(pn_h.data(), d_pn, (size_t)n * 4, hipMemcpyDeviceToHost));
    const float pn_max = *std::max_element(pn_h.begin(), pn_h.end());
    IndexView view = idx->view();
    const size_t smem_g = (size_t)2 * kTM * kLDP * 4;
    for (uint32_t qb = 0; qb < nq; qb += QC) {
        const uint32_t qc = std::min(QC, nq - qb);
        const uint32_t qpad = (qc + kTM - 1) / kTM * kTM;
        HIPCHK(hipMemcpy(d_qup, queries + (size_t)qb * idx->dim, (size_t)qc * idx->dim * 4, hipMemcpyHostToDevice));
        CHK(metric.prepare(d_qup, d_qnat, d_sq, qc, st, nullptr));
        HIPCHK(hipMemset(d_qb, 0, (size_t)qpad * stride * 4));
        {
            const size_t total = (size_t)qc * stride;
            const int grid = (int)std::min<size_t>((total + 255) / 256, 65536);
            IDIST_LAUNCH(permute_rows_kernel, grid, 256, 0, st, d_qnat, d_qb, qc, idx->kdim, stride, idx->L.nb);
        }
        IDIST_LAUNCH(row_norms_kernel, std::min<uint32_t>(qpad, 8192), 64, 0, st, d_qb, qpad, stride, d_qn);
        MfmaArgs a{};
        a.Q = d_qb; a.P = idx->d_points; a.qn = d_qn; a.pn = d_pn;
        a.nq = qc; a.n = n; a.stride = stride;
        a.dense = d_dense; a.dense_ld = S_pad; a.thr = d_thr; a.cand = d_cand; a.cnt = d_cnt; a.cap = cap;
        const uint32_t nqt = qpad / kTM;
        // pass 1: dense distances to the sample [0, S) -> per-query threshold
        a.mode = 0; a.p_begin = 0; a.p_end = S;
        IDIST_LAUNCH(mfma_dist_kernel, nqt * (S_pad / kTN), 256, smem_g, st, a);
        IDIST_LAUNCH(kth_threshold_kernel, std::min<uint32_t>(qc, 8192), 64, (size_t)(k + 72) * 8, st, d_dense, S_pad, S, qc, k,
                     k + 72, d_qn, pn_max, stride, d_thr);
        // pass 2: all points, keep those under the threshold
        HIPCHK(hipMemsetAsync(d_cnt, 0, (size_t)qpad * 4, st));
        a.mode = 1; a.p_begin = 0; a.p_end = n;
        IDIST_LAUNCH(mfma_dist_kernel, nqt * ((n + kTN - 1) / kTN), 256, smem_g, st, a);
        // pass 3: canonical re-rank of the candidates
        const uint32_t wcap = topk_wcap(k);
        const size_t smem_r = (size_t)stride * 4 + (size_t)wcap * 8 + 2 * 64 * 4;
        const uint32_t gridr = std::min<uint32_t>(qc, (uint32_t)idx->n_cu * 16);
#define LAUNCH_RR(NB_, RS_, TAIL_)                                                                                   \
    {                                                                                                                \
        auto kR = rerank_kernel<NB_, RS_, TAIL_>;                                                                    \
        IDIST_LAUNCH(kR, gridr, 64, smem_r, st, view, d_qnat, qc, k, wcap, d_cand, d_cnt, cap, d_pid, d_dist, d_ovf); \
    }
        IDIST_DISPATCH(idx->L, LAUNCH_RR);
#undef LAUNCH_RR
        HIPCHK(hipGetLastError());
        if (!raw) CHK(metric.report(d_dist, d_sq, qc, k, st));
        HIPCHK(hipMemcpy(out_pid + (size_t)qb * k, d_pid, (size_t)qc * k * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out_dist + (size_t)qb * k, d_dist, (size_t)qc * k * 4, hipMemcpyDeviceToHost));
    }
    uint32_t ovf = 0;
    HIPCHK(hipMemcpy(&ovf, d_ovf, 4, hipMemcpyDeviceToHost));
    if (ovf) { *fell_back = 1; return fail(IDIST_ERR_INTERNAL, "MFMA filter: %u candidate lists overflowed", ovf); }
    return IDIST_OK;
}

static idist_status bruteforce_impl(const idist_index* idx, const float* queries, uint32_t nq, uint32_t k,
                                    uint32_t* out_pid, float* out_dist, bool raw) {
    if (!idx) return fail(IDIST_ERR_INVALID_ARG, "idx is null");
    if (nq == 0) return IDIST_OK;
    if (k == 0 || k > IDIST_MAX_EF) return fail(IDIST_ERR_INVALID_ARG, "k %u out of [1,%u]", k, IDIST_MAX_EF);
    if (!queries || !out_pid || !out_dist) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    // the -2QP^T contraction only pays when the batch is wide enough to be a dense GEMM
    bool mfma = nq >= 256 && idx->n >= 16384;
    if (const char* e = test_env("IDIST_BRUTEFORCE")) mfma = strcmp(e, "mfma") == 0 ? true : (strcmp(e, "scan") == 0 ? false : mfma);
    if (mfma && idx->n >= k && idx->n >= 128) {
        HIPCHK(hipSetDevice(idx->device));
        int fell_back = 0;
        idist_status s = bruteforce_mfma(idx, queries, nq, k, out_pid, out_dist, &fell_back, raw);
        if (s == IDIST_OK || !fell_back) return s;
    }
    return bruteforce_scan(idx, queries, nq, k, out_pid, out_dist, raw);
}

idist_status idist_bruteforce(const idist_index* idx, const float* queries, uint32_t nq, uint32_t k,
                              uint32_t* out_pid, float* out_dist) {
    return bruteforce_impl(idx, queries, nq, k, out_pid, out_dist, false);
}

// ---- the ef ladder over Hnsw::search, then an exact scan: what the restricted searches and the range
// ---- search (§4.9) share ----
extern "C++" {
namespace {

// `fn` enqueues kernels on the context's stream between two HIP events (kernel events on); ladder_times_resolve adds their
// durations to ctx->al_ms[which] once the call has synchronised the stream — no synchronisation of its own
template <typename F> idist_status ladder_timed(idist_search_ctx* ctx, int which, F fn) {
    const uint32_t u = ctx->al_ev_used;
    if (!ctx->knobs.events || u + 2 > idist_search_ctx::kAllowedEvents) return fn();
    for (uint32_t i = u; i < u + 2; i++)
        if (!ctx->al_ev[i]) HIPCHK(hipEventCreate(&ctx->al_ev[i]));
    HIPCHK(hipEventRecord(ctx->al_ev[u], ctx->stream));
    CHK(fn());
    HIPCHK(hipEventRecord(ctx->al_ev[u + 1], ctx->stream));
    ctx->al_ev_which[u / 2] = (uint8_t)which;
    ctx->al_ev_used = u + 2;
    return IDIST_OK;
}
idist_status ladder_times_resolve(idist_search_ctx* ctx) {
    for (uint32_t u = 0; u < ctx->al_ev_used; u += 2) {
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, ctx->al_ev[u], ctx->al_ev[u + 1]));
        ctx->al_ms[ctx->al_ev_which[u / 2]] += ms;
    }
    ctx->al_ev_used = 0;
    return IDIST_OK;
}

// the argument checks, each message once (the range search has no k: it checks max_rungs alone)
idist_status check_max_rungs(int32_t max_rungs) {
    if (max_rungs < -1) return fail(IDIST_ERR_INVALID_ARG, "max_rungs %d: -1 (the whole ladder) or a number of rungs >= 0", max_rungs);
    return IDIST_OK;
}
idist_status check_ladder_args(int32_t max_rungs, uint32_t k, uint32_t ef0) {
    CHK(check_max_rungs(max_rungs));
    if (k == 0 || k > IDIST_MAX_EF) return fail(IDIST_ERR_INVALID_ARG, "k %u out of [1,%u]", k, IDIST_MAX_EF);
    if (ef0 != 0 && k > ef0) return fail(IDIST_ERR_INVALID_ARG, "k %u > ef_search %u", k, ef0);
    return IDIST_OK;
}
// (nq == 0 is no error: the caller returns at once, whatever set_of says)
idist_status check_sets_args(uint32_t n_sets, const uint32_t* set_of, uint32_t nq) {
    if (n_sets == 0) return fail(IDIST_ERR_INVALID_ARG, "n_sets 0: at least one allowed set");
    if (nq == 0) return IDIST_OK;
    if (!set_of && n_sets != nq) return fail(IDIST_ERR_INVALID_ARG, "set_of is null (query q uses set q) but n_sets %u != nq %u", n_sets, nq);
    if (set_of)
        for (uint32_t q = 0; q < nq; q++)
            if (set_of[q] >= n_sets) return fail(IDIST_ERR_INVALID_ARG, "set_of[%u] = %u: query %u names a set outside [0,%u)", q, set_of[q], q, n_sets);
    return IDIST_OK;
}

// ---- attribute filters: the sets of a restricted call made on the device ----
// Where a restricted call's sets come from: the caller's bitmaps (over the ids of an index, or the global ids of a partitioned
// one), or an attribute and the call's distinct intervals.  set_of [nq] is never null once a call has resolved it.
struct SetsSource {
    const uint32_t* bits = nullptr;                      // HOST bitmaps [n_sets][(n + 31) / 32] ...
    const idist_attr* attr = nullptr;                    // ... or the values on the device and
    const uint32_t *lo = nullptr, *hi = nullptr;         //     the distinct intervals, HOST [n_sets]
    const uint32_t* prog = nullptr;                      // ... or the table on the device (attr) and the distinct conditions as a flat
    uint32_t n_clauses = 0, n_and = 0;                   //     program, HOST: clauses [n_clauses][3], and_lims [n_and + 1], or_lims [n_sets + 1]
    uint32_t n_sets = 0;
    const uint32_t* set_of = nullptr;
    size_t prog_words() const { return (size_t)n_clauses * 3u + n_and + 1u + n_sets + 1u; }
};

// the conditions of an attribute call: one for the batch or one per query, as a radius (nq == 0 is no error)
idist_status check_cond_args(const uint32_t* lo, const uint32_t* hi, uint32_t n_cond, uint32_t nq) {
    if (nq == 0) return IDIST_OK;
    if (n_cond != 1 && n_cond != nq) return fail(IDIST_ERR_INVALID_ARG, "n_cond %u: 1 (one condition for the batch) or nq = %u", n_cond, nq);
    if (!lo || !hi) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    return IDIST_OK;
}

// D, the distinct (lo, hi) pairs of a call in ascending order, and every query's index into it.  nq entries: host work.
struct AttrConds {
    std::vector<uint32_t> lo, hi, set_of;
    SetsSource source(const idist_attr* attr) const {
        SetsSource s;
        s.attr = attr; s.lo = lo.data(); s.hi = hi.data(); s.n_sets = (uint32_t)lo.size(); s.set_of = set_of.data();
        return s;
    }
};
void attr_group(const uint32_t* lo, const uint32_t* hi, uint32_t n_cond, uint32_t nq, AttrConds* g) {
    g->set_of.assign(nq, 0u);
    std::vector<std::pair<uint64_t, uint32_t>> keyed(n_cond);
    for (uint32_t i = 0; i < n_cond; i++) keyed[i] = {(uint64_t)lo[i] << 32 | hi[i], i};
    std::sort(keyed.begin(), keyed.end());
    for (uint32_t i = 0; i < n_cond; i++) {
        if (i == 0 || keyed[i].first != keyed[i - 1].first) {
            g->lo.push_back((uint32_t)(keyed[i].first >> 32));
            g->hi.push_back((uint32_t)keyed[i].first);
        }
        if (n_cond == nq) g->set_of[keyed[i].second] = (uint32_t)g->lo.size() - 1u;
    }
}

// ---- conditions over a table: an OR of ANDs of interval clauses per query ----
// lims [count + 1]: starts at 0 and never decreases
idist_status check_lims(const char* what, const uint32_t* lims, uint32_t count) {
    if (lims[0] != 0) return fail(IDIST_ERR_INVALID_ARG, "%s[0] = %u: the first limit is 0", what, lims[0]);
    for (uint32_t i = 0; i < count; i++)
        if (lims[i + 1] < lims[i])
            return fail(IDIST_ERR_INVALID_ARG, "%s[%u] = %u is below %s[%u] = %u: the limits never decrease", what, i + 1u, lims[i + 1], what, i, lims[i]);
    return IDIST_OK;
}

// the conditions of a match call: one for the batch or one per query, as a radius (nq == 0 is no error); every clause names a column
// of the table
idist_status check_match_args(const idist_attr_conds* conds, uint32_t nq, uint32_t n_cols) {
    if (nq == 0) return IDIST_OK;
    if (!conds) return fail(IDIST_ERR_INVALID_ARG, "conds is null");
    const uint32_t n_cond = conds->n_cond;
    if (n_cond != 1 && n_cond != nq) return fail(IDIST_ERR_INVALID_ARG, "n_cond %u: 1 (one condition for the batch) or nq = %u", n_cond, nq);
    if (!conds->and_lims || !conds->or_lims) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    CHK(check_lims("or_lims", conds->or_lims, n_cond));
    const uint32_t n_and = conds->or_lims[n_cond];
    CHK(check_lims("and_lims", conds->and_lims, n_and));
    if (conds->and_lims[n_and] && !conds->clauses) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    for (uint32_t c = 0; c < n_cond; c++)
        for (uint32_t i = conds->and_lims[conds->or_lims[c]]; i < conds->and_lims[conds->or_lims[c + 1]]; i++)
            if (conds->clauses[i].col >= n_cols)
                return fail(IDIST_ERR_INVALID_ARG, "condition %u, clause %u: col %u, but the table has %u column%s", c, i, conds->clauses[i].col, n_cols,
                            n_cols == 1 ? "" : "s");
    return IDIST_OK;
}

// D, the distinct conditions of a call, as the flat program attr_match_kernel reads, and every query's index into it.  The clauses
// of a conjunction are ordered by (col, lo, hi) first — AND commutes, and the kernel keeps a column's tile while consecutive clauses
// name it — and the ordered forms are what is compared: conditions equal as encoded are equal here, and share one bitmap.  In the
// program every other conjunction is written with its columns downwards, so that it starts on the column the last one ended on.
struct MatchConds {
    std::vector<uint32_t> prog, set_of;                  // prog: clauses [n_clauses][3], and_lims [n_and + 1], or_lims [n_sets + 1]
    uint32_t n_clauses = 0, n_and = 0, n_sets = 0;
    SetsSource source(const idist_attr* attr) const {
        SetsSource s;
        s.attr = attr; s.prog = prog.data(); s.n_clauses = n_clauses; s.n_and = n_and; s.n_sets = n_sets; s.set_of = set_of.data();
        return s;
    }
};
void match_group(const idist_attr_conds* conds, uint32_t n_cond, uint32_t nq, MatchConds* g) {
    g->set_of.assign(nq, 0u);
    const uint32_t *al = n_cond ? conds->and_lims : nullptr, *ol = n_cond ? conds->or_lims : nullptr;
    std::vector<idist_attr_clause> cl;
    if (n_cond && al[ol[n_cond]]) cl.assign(conds->clauses, conds->clauses + al[ol[n_cond]]);
    auto clause_less = [](const idist_attr_clause& a, const idist_attr_clause& b) {
        return a.col != b.col ? a.col < b.col : a.lo != b.lo ? a.lo < b.lo : a.hi < b.hi;
    };
    for (uint32_t j = 0; n_cond && j < ol[n_cond]; j++) std::sort(cl.begin() + al[j], cl.begin() + al[j + 1], clause_less);
    // a total order of the conditions: the number of conjunctions, their lengths, then their ordered clauses
    auto compare = [&](uint32_t a, uint32_t b) -> int {
        const uint32_t na = ol[a + 1] - ol[a], nb = ol[b + 1] - ol[b];
        if (na != nb) return na < nb ? -1 : 1;
        for (uint32_t j = 0; j < na; j++) {
            const uint32_t la = al[ol[a] + j + 1] - al[ol[a] + j], lb = al[ol[b] + j + 1] - al[ol[b] + j];
            if (la != lb) return la < lb ? -1 : 1;
        }
        const idist_attr_clause *pa = cl.data() + al[ol[a]], *pb = cl.data() + al[ol[b]];
        for (uint32_t i = 0, m = al[ol[a + 1]] - al[ol[a]]; i < m; i++) {
            if (clause_less(pa[i], pb[i])) return -1;
            if (clause_less(pb[i], pa[i])) return 1;
        }
        return 0;
    };
    std::vector<uint32_t> order(n_cond);
    for (uint32_t i = 0; i < n_cond; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return compare(a, b) < 0; });
    std::vector<uint32_t> clauses, and_lims(1, 0u), or_lims(1, 0u);
    for (uint32_t i = 0; i < n_cond; i++) {
        const uint32_t c = order[i];
        if (i == 0 || compare(order[i - 1], c) != 0) {
            for (uint32_t j = ol[c]; j < ol[c + 1]; j++) {
                // every other conjunction of the program names its columns downwards: it starts on the column the one before it
                // ended on, whose tile the kernel still holds ("tenant = t AND day in [a, b]" per query: three loads per two conditions)
                const bool down = (and_lims.size() & 1u) == 0;
                for (uint32_t x = 0, m = al[j + 1] - al[j]; x < m; x++) {
                    const idist_attr_clause& k = cl[down ? al[j + 1] - 1u - x : al[j] + x];
                    clauses.insert(clauses.end(), {k.col, k.lo, k.hi});
                }
                and_lims.push_back((uint32_t)(clauses.size() / 3u));
            }
            or_lims.push_back((uint32_t)and_lims.size() - 1u);
        }
        if (n_cond == nq) g->set_of[c] = (uint32_t)or_lims.size() - 2u;
    }
    g->n_clauses = (uint32_t)(clauses.size() / 3u);
    g->n_and = (uint32_t)and_lims.size() - 1u;
    g->n_sets = (uint32_t)or_lims.size() - 1u;
    g->prog = std::move(clauses);
    g->prog.insert(g->prog.end(), and_lims.begin(), and_lims.end());
    g->prog.insert(g->prog.end(), or_lims.begin(), or_lims.end());
}

// an attribute belongs to ONE handle, as a context does: the index (partitioned == false) or the partitioned index with this uid
idist_status check_attr(const idist_attr* a, uint64_t uid, bool partitioned) {
    if (!a) return fail(IDIST_ERR_INVALID_ARG, "attr is null");
    if (a->partitioned != partitioned)
        return fail(IDIST_ERR_INVALID_ARG, partitioned ? "attr was made for an index, not for a partitioned index (idist_partitioned_attr_new)"
                                                       : "attr was made for a partitioned index, not for an index (idist_attr_new)");
    if (a->owner_uid != uid) return fail(IDIST_ERR_INVALID_ARG, partitioned ? "attr does not belong to this partitioned index" : "attr does not belong to idx");
    return IDIST_OK;
}

// attr_bitmaps_kernel on `stream` (its device is current): n >= 1, n_sets >= 1.  Work item = (tile of 4096 points, chunk of sets): one
// chunk — v read once — as soon as the tiles alone give every CU eight waves; never chunks of fewer than eight sets.
struct AttrGrid {
    uint32_t set_chunk, grid;
};
AttrGrid attr_grid(uint32_t n, uint32_t n_sets, int n_cu) {
    const uint64_t tiles = ((uint64_t)n + kAttrTile - 1u) / kAttrTile, want = (uint64_t)std::max(n_cu, 1) * 8u;
    const uint64_t chunks_wanted = std::max<uint64_t>((want + tiles - 1u) / tiles, 1u);
    const uint32_t set_chunk = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n_sets + chunks_wanted - 1u) / chunks_wanted, 8u), n_sets);
    const uint64_t items = tiles * ((n_sets + set_chunk - 1u) / set_chunk);
    return {set_chunk, (uint32_t)std::min<uint64_t>(items, (uint64_t)std::max(n_cu, 1) * 32u)};
}
idist_status launch_attr_bitmaps(const uint32_t* d_v, uint32_t n, const uint32_t* d_lo, const uint32_t* d_hi, uint32_t n_sets, uint32_t* d_out,
                                 int n_cu, hipStream_t stream) {
    const AttrGrid g = attr_grid(n, n_sets, n_cu);
    IDIST_LAUNCH(attr_bitmaps_kernel, g.grid, 64, 0, stream, d_v, n, d_lo, d_hi, n_sets, g.set_chunk, d_out);
    HIPCHK(hipGetLastError());
    return IDIST_OK;
}
// attr_match_kernel on `stream`, divided as launch_attr_bitmaps divides: d_v [n_cols][col_pitch], the program of n_sets conditions
// in device memory.  n >= 1, n_sets >= 1, col_pitch >= n.
idist_status launch_attr_match(const uint32_t* d_v, uint32_t n, uint32_t n_cols, uint64_t col_pitch, const AttrClause* d_clauses,
                               const uint32_t* d_and_lims, const uint32_t* d_or_lims, uint32_t n_sets, uint32_t* d_out, int n_cu,
                               hipStream_t stream) {
    const AttrGrid g = attr_grid(n, n_sets, n_cu);
    IDIST_LAUNCH(attr_match_kernel, g.grid, 64, 0, stream, d_v, n, n_cols, col_pitch, d_clauses, d_and_lims, d_or_lims, n_sets, g.set_chunk, d_out);
    HIPCHK(hipGetLastError());
    return IDIST_OK;
}

// The bitmaps of an attribute call into ctx->al_bits, on the context's stream (its device is current): the distinct intervals go
// up (or the distinct conditions over a table, as one program), the kernel runs between the context's own pair of events.  d_values
// [n_cols][n], n >= 1: the interval kernel reads column 0.  Staging: n_sets * ((n + 31) / 32) * 4 bytes.
idist_status attr_stage_bitmaps(idist_search_ctx* ctx, const uint32_t* d_values, uint32_t n, const SetsSource& src) {
    const size_t words = ((size_t)n + 31u) / 32u;
    hipStream_t stream = ctx->stream;
    CHK(ctx->al_bits.grow((size_t)src.n_sets * words * 4));
    if (src.prog) {
        CHK(ctx->at_prog.grow(src.prog_words() * 4));
        HIPCHK(hipMemcpyAsync(ctx->at_prog.p, src.prog, src.prog_words() * 4, hipMemcpyHostToDevice, stream));
    } else {
        CHK(ctx->at_lo.grow((size_t)src.n_sets * 4));
        CHK(ctx->at_hi.grow((size_t)src.n_sets * 4));
        HIPCHK(hipMemcpyAsync(ctx->at_lo.p, src.lo, (size_t)src.n_sets * 4, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(ctx->at_hi.p, src.hi, (size_t)src.n_sets * 4, hipMemcpyHostToDevice, stream));
    }
    ctx->at_timed = false;
    if (ctx->knobs.events) {
        for (hipEvent_t& e : ctx->at_ev)
            if (!e) HIPCHK(hipEventCreate(&e));
        HIPCHK(hipEventRecord(ctx->at_ev[0], stream));
    }
    if (src.prog) {
        const uint32_t *d_and = ctx->at_prog + (size_t)src.n_clauses * 3u, *d_or = d_and + src.n_and + 1u;
        CHK(launch_attr_match(d_values, n, src.attr->n_cols, n, reinterpret_cast<const AttrClause*>(ctx->at_prog.p), d_and, d_or, src.n_sets,
                              ctx->al_bits, ctx->n_cu, stream));
    } else {
        CHK(launch_attr_bitmaps(d_values, n, ctx->at_lo, ctx->at_hi, src.n_sets, ctx->al_bits, ctx->n_cu, stream));
    }
    if (ctx->knobs.events) {
        HIPCHK(hipEventRecord(ctx->at_ev[1], stream));
        ctx->at_timed = true;                            // (both recorded: attr_time_resolve may ask for their distance)
    }
    return IDIST_OK;
}
// ... and its time, once the call has synchronised the stream
idist_status attr_time_resolve(idist_search_ctx* ctx) {
    if (!ctx->at_timed) return IDIST_OK;
    ctx->at_timed = false;
    HIPCHK(hipEventElapsedTime(&ctx->at_ms, ctx->at_ev[0], ctx->at_ev[1]));
    return IDIST_OK;
}

// The sets of a several-sets call on ONE index, on the context's stream: al_bits — the caller's bitmaps as they are (padding bits are
// masked where they are read), or the attribute's, made here — and al_setof.  n >= 1.
idist_status stage_sets(idist_search_ctx* ctx, uint32_t n, uint32_t nq, const SetsSource& src) {
    const size_t bb = (size_t)src.n_sets * (((size_t)n + 31u) / 32u) * 4;
    CHK(ctx->al_setof.grow((size_t)nq * 4));
    if (src.attr) {
        CHK(attr_stage_bitmaps(ctx, src.attr->parts[0].v, n, src));
    } else {
        CHK(ctx->al_bits.grow(bb));
        HIPCHK(hipMemcpyAsync(ctx->al_bits.p, src.bits, bb, hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(hipMemcpyAsync(ctx->al_setof.p, src.set_of, (size_t)nq * 4, hipMemcpyHostToDevice, ctx->stream));
    return IDIST_OK;
}

// step 1, nothing to find: every output array the caller hands in (null: it has none, or fills it its own way)
void fill_nothing_found(uint32_t nq, uint32_t k, uint32_t* out_pid, float* out_dist, uint32_t* out_count, uint32_t* out_rung,
                        uint32_t* out_counters) {
    if (out_pid) std::fill(out_pid, out_pid + (size_t)nq * k, (uint32_t)IDIST_INVALID);
    if (out_dist) std::fill(out_dist, out_dist + (size_t)nq * k, INFINITY);
    if (out_count) memset(out_count, 0, (size_t)nq * 4);
    if (out_rung) std::fill(out_rung, out_rung + nq, (uint32_t)IDIST_RUNG_NONE);
    if (out_counters) memset(out_counters, 0, (size_t)nq * 12);
}

// the ladder E[0] = ef_search, E[r + 1] = min(4 E[r], IDIST_MAX_EF), ending with the rung that equals IDIST_MAX_EF; the permitted
// rungs are r < n_rungs.  ef0 > 0.
AllowedLadder make_ladder(uint32_t ef0, int32_t max_rungs) {
    AllowedLadder lad{};
    for (uint32_t e = ef0;; e = std::min<uint32_t>(4u * e, IDIST_MAX_EF)) {
        lad.E[lad.n_rungs++] = e;
        if (e >= IDIST_MAX_EF) break;
    }
    if (max_rungs >= 0) lad.n_rungs = std::min<uint32_t>(lad.n_rungs, (uint32_t)max_rungs);
    return lad;
}

// *d_qk [nq][kdim]: the queries as the kernels read them.  Cosine / DOT: prepared ONCE per call, every rung and the exact scan take
// them as they are (prepared = true), and the caller reports once, on the call's result — as the partitioned search does
idist_status ladder_upload_queries(const idist_index* idx, idist_search_ctx* ctx, const MetricPasses& metric, const float* queries,
                                   uint32_t nq, const float** d_qk) {
    const size_t qb = (size_t)nq * idx->dim * 4;
    CHK(ctx->d_q.grow(qb));
    HIPCHK(hipMemcpyAsync(ctx->d_q, queries, qb, hipMemcpyHostToDevice, ctx->stream));
    *d_qk = ctx->d_q;
    if (metric.any()) {
        CHK(ctx->d_qn.grow(doubled_from(4096, metric.qk_floats(nq) * 4)));
        CHK(ctx->d_sq.grow(doubled_from(256, metric.sq_floats(nq) * 4)));
        CHK(metric.prepare(ctx->d_q, ctx->d_qn, ctx->d_sq, nq, ctx->stream, d_qk));
    }
    return IDIST_OK;
}

// One rung: Hnsw::search at `ef` for the queries d_pq [np][kdim] into ctx->d_pid / d_dist [np][ef], d_cnt, d_ctr; blocks on the
// context's stream.  *ended: the ladder is over, nothing was launched.
idist_status ladder_rung(const idist_index* idx, idist_search_ctx* ctx, const float* d_pq, uint32_t np, uint32_t ef, uint32_t r,
                         bool counters, bool* ended) {
    *ended = false;
    const size_t rb = (size_t)np * ef * 4;
    CHK(ctx->d_pid.grow(rb));
    CHK(ctx->d_dist.grow(rb));
    CHK(ctx->d_cnt.grow((size_t)np * 4));
    CHK(ctx->d_ctr.grow((size_t)np * 12));
    for (;;) {
        bool lds_short = false;
        SearchOpts opts;
        opts.prepared = true;
        opts.ef = ef;
        opts.lds_short = &lds_short;
        const idist_status ls = launch_search(idx, ctx, d_pq, np, ctx->d_pid, ctx->d_dist, ctx->d_cnt, counters ? ctx->d_ctr.p : nullptr,
                                              ctx->stream, opts);
        if (ls != IDIST_OK) {
            // a later rung that does not fit a wave's LDS ends the ladder as max_rungs would; rung 0 fails as idist_search_batch does
            if (lds_short && r != 0) { *ended = true; return IDIST_OK; }
            return ls;
        }
        HIPCHK(hipStreamSynchronize(ctx->stream));
        idist_status s;
        if (status_asks_retry(idx, ctx, &s)) continue;          // strict ties: the same rung again with the larger region / the bags
        return s;
    }
}

// The pending pass, enqueued only: the pending queries (d_first: whose first rung is <= rung; d_last: whose last rung is > rung)
// ascending into list_out, their rows into ctx->al_pq, their number into ctx->al_npend — which the caller reads back (the range
// searches: with their new total, in one wait)
idist_status ladder_pending(idist_search_ctx* ctx, const uint32_t* pending, uint32_t nq, const float* d_qk, uint32_t kdim,
                            uint32_t* list_out, int which_timer, const uint32_t* d_first = nullptr, uint32_t rung = 0,
                            const uint32_t* d_last = nullptr) {
    auto pending_pass = [&]() -> idist_status {
        IDIST_LAUNCH(allowed_pending_kernel, (nq + 63u) / 64u, 64, 0, ctx->stream, pending, nq, d_qk, kdim, list_out, ctx->al_pq,
                     ctx->al_npend, d_first, rung, d_last);
        HIPCHK(hipGetLastError());
        return IDIST_OK;
    };
    return ladder_timed(ctx, which_timer, pending_pass);
}

// S of an exact step, `units` rows per pending query cut into S segments: enough waves for the chip when few queries are left,
// never segments of less than one 64-row round; the test knob overrides; at most 64.  The result does not depend on it.
uint32_t exact_segments(const idist_search_ctx* ctx, uint32_t np, uint64_t units, uint32_t knob) {
    static_assert(kMergeMaxLists == 64, "the range search's bound is the merge's");
    uint32_t S = (uint32_t)std::min<uint64_t>(((uint64_t)std::max(ctx->n_cu, 1) * 16u + np - 1u) / np, (units + 63u) / 64u);
    if (knob) S = knob;
    return std::min(std::max(S, 1u), kMergeMaxLists);
}

idist_status allowed_select(idist_search_ctx* ctx, const AllowedOut& o, uint32_t n, const uint32_t* r_pid, const float* r_dist,
                            const uint32_t* r_cnt, const uint32_t* r_ctr, uint32_t width, const uint32_t* list, uint32_t np,
                            uint32_t rung, bool exact, const uint32_t* set_of = nullptr, uint32_t words = 0) {
    auto select_pass = [&]() -> idist_status {
        const uint32_t grid = std::min<uint32_t>(np, 65536u);                 // one wave per pending query; the kernel strides over the rest
        IDIST_LAUNCH(allowed_select_kernel, grid, 64, 0, ctx->stream, o, ctx->al_bits, n, r_pid,
                     reinterpret_cast<const uint32_t*>(r_dist), r_cnt, r_ctr, width, list, np, rung, exact ? 1u : 0u, set_of,
                     words);
        HIPCHK(hipGetLastError());
        return IDIST_OK;
    };
    return ladder_timed(ctx, 0, select_pass);
}

// The scan and merge half of an exact step, around either scan kernel: launch_scan enqueues one wave per (pending query, segment),
// each writing its segment's top-k as list s of the merge by (distance bits, id); the k best of every pending query end up in
// ctx->al_mpid / al_mdist [np][k], al_mcnt [np]
template <typename F>
idist_status exact_scan_merge(const idist_index* idx, idist_search_ctx* ctx, uint32_t np, uint32_t k, uint32_t S, F launch_scan) {
    const size_t sb = (size_t)S * np * k * 4, mb = (size_t)np * k * 4;
    CHK(ctx->d_pid.grow(sb));
    CHK(ctx->d_dist.grow(sb));
    CHK(ctx->d_cnt.grow((size_t)S * np * 4));
    CHK(ctx->al_mpid.grow(mb));
    CHK(ctx->al_mdist.grow(mb));
    CHK(ctx->al_mcnt.grow((size_t)np * 4));
    const uint32_t wcap = topk_wcap(k);
    const size_t smem = smem_bytes(idx->L.stride, wcap, false);
    if (smem > 64 * 1024) return fail(IDIST_ERR_INVALID_ARG, "dim/k need %zu B of LDS per wave (> 64 KiB)", smem);
    auto scan_and_merge = [&]() -> idist_status {
        const uint32_t grid = (uint32_t)std::min<uint64_t>((uint64_t)np * S, (uint64_t)std::max(ctx->n_cu, 1) * 64u);
        uint32_t *s_pid = ctx->d_pid, *s_dist = reinterpret_cast<uint32_t*>(ctx->d_dist.p), *s_cnt = ctx->d_cnt;
        launch_scan(grid, smem, S, wcap, s_pid, s_dist, s_cnt);
        HIPCHK(hipGetLastError());
        MergeArgs a{};
        a.pid = s_pid; a.dist = s_dist; a.count = s_cnt; a.counters = nullptr;
        a.n_lists = S; a.nq = np; a.width = k; a.out_width = k;
        a.out_pid = ctx->al_mpid; a.out_dist = ctx->al_mdist.as<uint32_t>(); a.out_count = ctx->al_mcnt;
        a.out_counters = nullptr;
        return launch_merge(a, ctx->stream);
    };
    return ladder_timed(ctx, 2, scan_and_merge);
}

// Step 5 of the restricted search, exact: the k best of the scan are selected as rung IDIST_RUNG_EXACT
template <typename F>
idist_status allowed_exact_step(const idist_index* idx, idist_search_ctx* ctx, const AllowedOut& o, uint32_t np, uint32_t k, uint32_t S,
                                const uint32_t* d_list, const uint32_t* d_setof, uint32_t words, F launch_scan) {
    CHK(exact_scan_merge(idx, ctx, np, k, S, launch_scan));
    return allowed_select(ctx, o, idx->n, ctx->al_mpid, ctx->al_mdist.as<float>(), ctx->al_mcnt, nullptr, k,
                          d_list, np, IDIST_RUNG_EXACT, true, d_setof, words);
}

// a call's [nq][k] result with its counts, rungs and counters in the context's own memory
idist_status allowed_out_in_ctx(idist_search_ctx* ctx, uint32_t nq, uint32_t k, bool counters, AllowedOut* o) {
    const size_t ob = (size_t)nq * k * 4;
    CHK(ctx->al_opid.grow(ob));
    CHK(ctx->al_odist.grow(ob));
    CHK(ctx->al_ocnt.grow((size_t)nq * 4));
    CHK(ctx->al_orung.grow((size_t)nq * 4));
    CHK(ctx->al_octr.grow((size_t)nq * 12));
    o->pid = ctx->al_opid; o->dist = ctx->al_odist.as<uint32_t>(); o->count = ctx->al_ocnt;
    o->rung = ctx->al_orung; o->counters = counters ? ctx->al_octr.p : nullptr;
    return IDIST_OK;
}
// ... and its way back to the caller, enqueued: the caller synchronises the stream and calls ladder_times_resolve
idist_status allowed_download(idist_search_ctx* ctx, uint32_t nq, uint32_t k, uint32_t* out_pid, float* out_dist, uint32_t* out_count,
                              uint32_t* out_rung, uint32_t* out_counters) {
    const size_t ob = (size_t)nq * k * 4;
    HIPCHK(hipMemcpyAsync(out_pid, ctx->al_opid.p, ob, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(out_dist, ctx->al_odist.p, ob, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(out_count, ctx->al_ocnt.p, (size_t)nq * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (out_rung) HIPCHK(hipMemcpyAsync(out_rung, ctx->al_orung.p, (size_t)nq * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (out_counters) HIPCHK(hipMemcpyAsync(out_counters, ctx->al_octr.p, (size_t)nq * 12, hipMemcpyDeviceToHost, ctx->stream));
    return IDIST_OK;
}

}  // namespace
}  // extern "C++"

// ---- restricted search: the ladder filtered by an allowed set, exact scan of the allowed rows ----
// (not the several-sets call with n_sets = 1: the bitmap scan, a count pass and one more synchronisation are a speed nobody has measured)
idist_status idist_search_batch_allowed(const idist_index* idx, idist_search_ctx* ctx, const float* queries, uint32_t nq,
                                        const uint32_t* allow_bits, uint32_t k, int32_t max_rungs, uint32_t* out_pid,
                                        float* out_dist, uint32_t* out_count, uint32_t* out_rung, uint32_t* out_counters) {
    CHK(check_ctx(idx, ctx));
    const uint32_t n = idx->n, ef0 = idx->cfg.ef_search;
    CHK(check_ladder_args(max_rungs, k, ef0));
    if (nq == 0) return IDIST_OK;
    if (!queries || !out_pid || !out_dist || !out_count || (n && !allow_bits)) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    // A: the bitmap with the bits at positions >= n cleared, its size, and (when an exact step needs it) its ascending id list
    const uint32_t words = (n + 31u) / 32u;
    std::vector<uint32_t> bits(allow_bits, allow_bits + words);
    if (n % 32u) bits[words - 1] &= (1u << (n % 32u)) - 1u;
    uint64_t n_allowed = 0;
    for (const uint32_t w : bits) n_allowed += (uint64_t)__builtin_popcount(w);
    if (n == 0 || ef0 == 0 || n_allowed == 0) {                              // step 1: nothing to find
        fill_nothing_found(nq, k, out_pid, out_dist, out_count, out_rung, out_counters);
        return IDIST_OK;
    }
    // the start rung is the first permitted one whose expected number of allowed hits reaches k (64-bit)
    const AllowedLadder lad = make_ladder(ef0, max_rungs);
    uint32_t r0 = lad.n_rungs;
    if (n_allowed > k)
        for (uint32_t r = 0; r < lad.n_rungs && r0 == lad.n_rungs; r++)
            if ((uint64_t)lad.E[r] * n_allowed >= (uint64_t)k * n) r0 = r;

    HIPCHK(hipSetDevice(idx->device));
    hipStream_t stream = ctx->stream;
    const MetricPasses metric(idx);
    const uint32_t kdim = idx->kdim;
    const bool counters = out_counters != nullptr;
    ctx->al_ms[0] = ctx->al_ms[1] = ctx->al_ms[2] = 0.0f;
    ctx->al_ev_used = 0;
    CHK(ctx->al_bits.grow((size_t)words * 4));
    CHK(ctx->al_flag.grow((size_t)nq * 4));
    CHK(ctx->al_list.grow((size_t)nq * 4));
    CHK(ctx->al_npend.grow(256));
    CHK(ctx->al_pq.grow((size_t)nq * kdim * 4));
    AllowedOut o{};
    CHK(allowed_out_in_ctx(ctx, nq, k, counters, &o));
    o.pending = ctx->al_flag; o.nq = nq; o.k = k;
    HIPCHK(hipMemcpyAsync(ctx->al_bits.p, bits.data(), (size_t)words * 4, hipMemcpyHostToDevice, stream));
    const float* d_qk = nullptr;
    CHK(ladder_upload_queries(idx, ctx, metric, queries, nq, &d_qk));
    {
        const uint32_t grid = (uint32_t)std::min<size_t>(((size_t)nq * k + 255) / 256, (size_t)std::max(ctx->n_cu, 1) * 8u);
        IDIST_LAUNCH(allowed_init_kernel, grid, 256, 0, stream, o);
        HIPCHK(hipGetLastError());
    }
    // the pending queries: all of them, in place, until the first rung has answered some
    uint32_t np = nq;
    std::vector<uint32_t> ids;                                   // (lives until the last synchronisation: it is uploaded asynchronously)
    const uint32_t* d_list = nullptr;
    const float* d_pq = d_qk;
    for (uint32_t r = r0; r < lad.n_rungs && np; r++) {
        const uint32_t ef = lad.E[r];
        bool ended = false;
        CHK(ladder_rung(idx, ctx, d_pq, np, ef, r, counters, &ended));
        if (ended) break;
        CHK(allowed_select(ctx, o, n, ctx->d_pid, ctx->d_dist, ctx->d_cnt, counters ? ctx->d_ctr.p : nullptr, ef, d_list, np, r, false));
        CHK(ladder_pending(ctx, o.pending, nq, d_qk, kdim, ctx->al_list, 1));
        HIPCHK(hipMemcpyAsync(&np, ctx->al_npend.p, 4, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        d_list = ctx->al_list;
        d_pq = ctx->al_pq;
    }
    if (np) {
        // step 5, exact: the ascending id list of A cut into S segments, the segments' top-k lists merged
        ids.reserve((size_t)n_allowed);
        for (uint32_t w = 0; w < words; w++)
            for (uint32_t m = bits[w]; m; m &= m - 1u) ids.push_back(32u * w + (uint32_t)__builtin_ctz(m));
        const uint32_t n_ids = (uint32_t)ids.size();
        CHK(ctx->al_ids.grow((size_t)n_ids * 4));
        HIPCHK(hipMemcpyAsync(ctx->al_ids.p, ids.data(), (size_t)n_ids * 4, hipMemcpyHostToDevice, stream));
        const uint32_t* d_ids = ctx->al_ids;
        const IndexView view = idx->view();
        auto scan_ids = [&](uint32_t grid, size_t smem, uint32_t S, uint32_t wcap, uint32_t* s_pid, uint32_t* s_dist, uint32_t* s_cnt) {
#define LAUNCH_AS(NB_, RS_, TAIL_)                                                                                        \
    {                                                                                                                     \
        auto kA = allowed_scan_kernel<NB_, RS_, TAIL_>;                                                                   \
        IDIST_LAUNCH(kA, grid, 64, smem, stream, view, d_pq, np, d_ids, n_ids, S, k, wcap, s_pid, s_dist, s_cnt);          \
    }
            IDIST_DISPATCH(idx->L, LAUNCH_AS);
#undef LAUNCH_AS
        };
        CHK(allowed_exact_step(idx, ctx, o, np, k, exact_segments(ctx, np, n_ids, ctx->knobs.allowed_segments), d_list, nullptr, 0, scan_ids));
    }
    CHK(metric.report(ctx->al_odist.as<float>(), ctx->d_sq, nq, k, stream));
    CHK(allowed_download(ctx, nq, k, out_pid, out_dist, out_count, out_rung, out_counters));
    HIPCHK(hipStreamSynchronize(stream));
    return ladder_times_resolve(ctx);
}

extern "C++" {
namespace {

// The several-sets call between its uploads and its report: everything already in the memory of the index's device (which is
// current).  d_qk [nq][kdim]: the queries as the kernels read them (MetricPasses::prepare has run, or the metric has none); d_bits
// [n_sets][(n + 31) / 32]; d_setof [nq] and its host copy set_of (never null here).  o.pid / dist / count / rung / counters: where the
// [nq][k] result goes, RAW distances — the caller reports; o.pending is set here.  n > 0, ef_search > 0, nq > 0 and the arguments
// checked.  Blocks on ctx->stream once per rung; on return the last passes are enqueued there, not waited for: the caller
// synchronises the stream and calls ladder_times_resolve.
// What is done with a rung's lists and what the exact step is are the caller's (the restricted search filters and scans, the grouped
// search collapses and scans in rounds):
//   select_rung(o, ef, d_list, np, r)           the np lists of rung r in ctx->d_pid / d_dist [np][ef], d_cnt, d_ctr; d_list: the
//                                               query of every list (nullptr: the identity)
//   exact_step(o, d_list, d_pq, np, gather)     the np queries still pending, their rows in d_pq; gather(kRungExact) makes the three
//                                               anew from o.pending
// known_start [n_sets] (host; nullptr: counted here): the first step of every set by the start rule, where the caller knows |A_s|.
template <typename Select, typename Exact>
idist_status sets_ladder_device(const idist_index* idx, idist_search_ctx* ctx, const float* d_qk, uint32_t nq, const uint32_t* d_bits,
                                uint32_t n_sets, const uint32_t* d_setof, const uint32_t* set_of, uint32_t k, int32_t max_rungs,
                                AllowedOut o, Select select_rung, Exact exact_step, const uint32_t* known_start = nullptr) {
    const uint32_t n = idx->n;
    // the permitted rungs, as idist_search_batch_allowed has them; every set's size and start rung come from the device
    const uint32_t words = (n + 31u) / 32u;
    const AllowedLadder lad = make_ladder(idx->cfg.ef_search, max_rungs);
    const uint32_t n_rungs = lad.n_rungs;
    hipStream_t stream = ctx->stream;
    const uint32_t kdim = idx->kdim;
    const bool counters = o.counters != nullptr;
    ctx->al_ms[0] = ctx->al_ms[1] = ctx->al_ms[2] = 0.0f;
    ctx->al_ev_used = 0;
    CHK(ctx->al_size.grow((size_t)n_sets * 4));
    CHK(ctx->al_start.grow((size_t)n_sets * 4));
    CHK(ctx->al_first.grow((size_t)nq * 4));
    CHK(ctx->al_flag.grow((size_t)nq * 4));
    CHK(ctx->al_list.grow((size_t)nq * 4));
    CHK(ctx->al_npend.grow(256));
    CHK(ctx->al_pq.grow((size_t)nq * kdim * 4));
    o.pending = ctx->al_flag; o.nq = nq; o.k = k;
    const uint32_t* d_first = ctx->al_first;
    auto count_pass = [&]() -> idist_status {
        const uint32_t grid = std::min<uint32_t>(n_sets, (uint32_t)std::max(ctx->n_cu, 1) * 32u);
        IDIST_LAUNCH(allowed_count_kernel, grid, 64, 0, stream, d_bits, n, words, n_sets, k, lad, ctx->al_size,
                     ctx->al_start);
        HIPCHK(hipGetLastError());
        return IDIST_OK;
    };
    std::vector<uint32_t> start(n_sets);
    if (known_start) {                                   // the caller knows every set's first step (d_bits may be null): no count pass
        start.assign(known_start, known_start + n_sets);
        HIPCHK(hipMemcpyAsync(ctx->al_start.p, start.data(), (size_t)n_sets * 4, hipMemcpyHostToDevice, stream));
    } else {
        CHK(ladder_timed(ctx, 0, count_pass));
        HIPCHK(hipMemcpyAsync(start.data(), ctx->al_start.p, (size_t)n_sets * 4, hipMemcpyDeviceToHost, stream));
    }
    {
        const uint32_t grid = (uint32_t)std::min<size_t>(((size_t)nq * k + 255) / 256, (size_t)std::max(ctx->n_cu, 1) * 8u);
        IDIST_LAUNCH(allowed_init_kernel, grid, 256, 0, stream, o, ctx->al_start, d_setof, ctx->al_first);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(stream));
    // how many queries start on which rung: what tells "nobody runs this rung, but some are still waiting" from "nobody is left"
    uint32_t starts[8] = {0}, n_exact = 0;
    for (uint32_t q = 0; q < nq; q++) {
        const uint32_t f = start[set_of[q]];
        if (f < 8u) starts[f]++;
        else if (f == kRungExact) n_exact++;
    }
    auto next_start = [&](uint32_t from) {                      // the first rung >= from some query starts on (n_rungs: none)
        while (from < n_rungs && !starts[from]) from++;
        return std::min(from, n_rungs);
    };
    auto waiting_after = [&](uint32_t r) {                      // queries whose first step comes after rung r
        uint32_t w = n_exact;
        for (uint32_t i = r + 1u; i < n_rungs; i++) w += starts[i];
        return w;
    };
    // the queries of a launch: the pending ones whose first rung has come up (rung kRungExact: everything still pending), ascending
    uint32_t np = 0;
    const uint32_t* d_list = nullptr;
    const float* d_pq = d_qk;
    auto gather = [&](uint32_t rung) -> idist_status {
        CHK(ladder_pending(ctx, o.pending, nq, d_qk, kdim, ctx->al_list, 1, d_first, rung));
        HIPCHK(hipMemcpyAsync(&np, ctx->al_npend.p, 4, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        d_list = ctx->al_list;
        d_pq = ctx->al_pq;
        return IDIST_OK;
    };
    uint32_t r = next_start(0);
    bool all_done = false;
    // every query on the same first step: the batch as it is, in place, as the single-set call launches it
    bool in_place = (r < n_rungs && starts[r] == nq) || n_exact == nq;
    if (in_place) np = nq;
    while (r < n_rungs) {
        if (!in_place) {
            CHK(gather(r));
            if (!np) {
                if (!waiting_after(r)) { all_done = true; break; }
                r = next_start(r + 1u);                          // nobody runs this rung, the waiting ones start later
                continue;
            }
        }
        in_place = false;
        const uint32_t ef = lad.E[r];
        bool ended = false;
        CHK(ladder_rung(idx, ctx, d_pq, np, ef, r, counters, &ended));
        if (ended) break;
        CHK(select_rung(o, ef, d_list, np, r));
        r++;
    }
    if (!all_done && !in_place) CHK(gather(kRungExact));
    if (!all_done && np) CHK(exact_step(o, d_list, d_pq, np, gather));
    return IDIST_OK;
}

// an exact scan straight from bitmaps: the pending rows d_pq [np][kdim] of the queries list [np] (nullptr: the identity), query q
// reading d_bits + set_of[q] * words — what exact_scan_merge takes as launch_scan
auto scan_bits_launcher(const idist_index* idx, hipStream_t stream, const float* d_pq, uint32_t np, const uint32_t* d_bits, uint32_t words,
                        const uint32_t* d_list, const uint32_t* d_setof, uint32_t k) {
    return [=](uint32_t grid, size_t smem, uint32_t S, uint32_t wcap, uint32_t* s_pid, uint32_t* s_dist, uint32_t* s_cnt) {
        const IndexView view = idx->view();
        const uint32_t n = idx->n;
#define LAUNCH_AS(NB_, RS_, TAIL_)                                                                                                 \
    {                                                                                                                              \
        auto kA = allowed_scan_bits_kernel<NB_, RS_, TAIL_>;                                                                       \
        IDIST_LAUNCH(kA, grid, 64, smem, stream, view, d_pq, np, d_bits, n, words, d_list, d_setof, S, k, wcap, s_pid, s_dist, s_cnt); \
    }
        IDIST_DISPATCH(idx->L, LAUNCH_AS);
#undef LAUNCH_AS
    };
}

// The several-sets call: a rung's lists filtered by the query's set; step 5, exact, straight from the bitmaps — the 64-id windows of
// [0, n) cut into S segments, never narrower than one window
idist_status allowed_sets_device(const idist_index* idx, idist_search_ctx* ctx, const float* d_qk, uint32_t nq, const uint32_t* d_bits,
                                 uint32_t n_sets, const uint32_t* d_setof, const uint32_t* set_of, uint32_t k, int32_t max_rungs,
                                 AllowedOut o) {
    const uint32_t n = idx->n, words = (n + 31u) / 32u;
    auto select_rung = [&](const AllowedOut& out, uint32_t ef, const uint32_t* d_list, uint32_t np, uint32_t r) {
        return allowed_select(ctx, out, n, ctx->d_pid, ctx->d_dist, ctx->d_cnt, out.counters ? ctx->d_ctr.p : nullptr, ef, d_list, np, r, false,
                              d_setof, words);
    };
    auto exact_step = [&](const AllowedOut& out, const uint32_t*& d_list, const float*& d_pq, uint32_t& np, auto&) {
        return allowed_exact_step(idx, ctx, out, np, k, exact_segments(ctx, np, n, ctx->knobs.allowed_segments), d_list, d_setof, words,
                                  scan_bits_launcher(idx, ctx->stream, d_pq, np, d_bits, words, d_list, d_setof, k));
    };
    return sets_ladder_device(idx, ctx, d_qk, nq, d_bits, n_sets, d_setof, set_of, k, max_rungs, o, select_rung, exact_step);
}

// ---- grouped search: the ladder collapsed by a column, exact rounds ----
// grouped_select_kernel on `stream` over np lists of `width`; d_bits null: every id < n is allowed
idist_status launch_grouped_select(const GroupedOut& g, const uint32_t* d_groups, uint32_t n, const uint32_t* d_bits, uint32_t words,
                                   const uint32_t* d_setof, const uint32_t* r_pid, const uint32_t* r_dist, const uint32_t* r_cnt,
                                   const uint32_t* r_ctr, uint32_t width, const uint32_t* d_list, uint32_t np, uint32_t rung, uint32_t mode,
                                   hipStream_t stream) {
    const uint32_t tab_log2 = grouped_tab_log2(g.k);
    const uint32_t grid = std::min<uint32_t>(np, 65536u);                     // one wave per list; the kernel strides over the rest
    IDIST_LAUNCH(grouped_select_kernel, grid, 64, (size_t)8u << tab_log2, stream, g, d_groups, n, d_bits, words, d_setof, r_pid, r_dist, r_cnt,
                 r_ctr, width, d_list, np, rung, mode, tab_log2);
    HIPCHK(hipGetLastError());
    return IDIST_OK;
}

// The exact step of the grouped search, in rounds: for the pending queries one bitmap each, A and "group not found yet"; the scan and
// merge of the restricted search give the k nearest remaining points; the collapse appends their new groups.  A query closes when
// its count reaches k or its list came back shorter than k.  Every remaining point nearer than a kept entry is in the list in front
// of it, so the found groups are a prefix of the true group order after every round: the result depends neither on the width of a
// round nor on S nor on the chunks, and a round adds at least one group to every query it leaves pending — at most k rounds.  The
// bitmaps of a chunk of pending queries stay under a fixed staging bound.
template <typename Gather>
idist_status grouped_exact_rounds(const idist_index* idx, idist_search_ctx* ctx, const GroupedOut& g, const uint32_t* d_groups,
                                  const uint32_t* d_bits, const uint32_t* d_setof, const uint32_t*& d_list, const float*& d_pq, uint32_t& np,
                                  Gather& gather) {
    const uint32_t n = idx->n, k = g.k, kdim = idx->kdim, words = (n + 31u) / 32u;
    const uint32_t tab_log2 = grouped_tab_log2(k);
    hipStream_t stream = ctx->stream;
    if (!d_list) CHK(gather(kRungExact));                                     // a chunk names its queries through the list
    const uint64_t bound = ctx->knobs.grouped_stage ? ctx->knobs.grouped_stage : (uint64_t)256u << 20;
    const uint32_t chunk = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(bound / ((uint64_t)words * 4u), 1u), np);
    CHK(ctx->gr_bits.grow((size_t)chunk * words * 4));
    CHK(ctx->gr_ident.grow((size_t)chunk * 4));
    for (uint32_t round = 0; np; round++) {
        if (round > k) return fail(IDIST_ERR_INTERNAL, "grouped search: %u queries still pending after %u exact rounds", np, round);
        for (uint32_t c0 = 0; c0 < np; c0 += chunk) {
            const uint32_t npc = std::min(chunk, np - c0);
            const uint32_t* lst = d_list + c0;
            auto exclude_pass = [&]() -> idist_status {
                const uint32_t S = exact_segments(ctx, npc, n, ctx->knobs.allowed_segments);    // (rows: at most one segment per window)
                const uint32_t grid = (uint32_t)std::min<uint64_t>((uint64_t)npc * S, (uint64_t)std::max(ctx->n_cu, 1) * 64u);
                IDIST_LAUNCH(grouped_exclude_kernel, grid, 64, (size_t)8u << tab_log2, stream, d_bits, n, words, d_setof, lst, npc, d_groups,
                             g.group, g.count, k, S, tab_log2, ctx->gr_bits, ctx->gr_ident);
                HIPCHK(hipGetLastError());
                return IDIST_OK;
            };
            CHK(ladder_timed(ctx, 2, exclude_pass));
            CHK(exact_scan_merge(idx, ctx, npc, k, exact_segments(ctx, npc, n, ctx->knobs.allowed_segments),
                                 scan_bits_launcher(idx, stream, d_pq + (size_t)c0 * kdim, npc, ctx->gr_bits, words, nullptr, ctx->gr_ident, k)));
            auto select_pass = [&]() -> idist_status {
                return launch_grouped_select(g, d_groups, n, nullptr, words, nullptr, ctx->al_mpid, ctx->al_mdist.as<uint32_t>(), ctx->al_mcnt,
                                             nullptr, k, lst, npc, IDIST_RUNG_EXACT, kGroupedRound, stream);
            };
            CHK(ladder_timed(ctx, 0, select_pass));
        }
        CHK(gather(kRungExact));
    }
    return IDIST_OK;
}

// The grouped call between its uploads and its report, as allowed_sets_device: the same count pass, init, pending pass and rungs;
// d_groups [n]: the group column; d_ogroup [nq][k]: the groups of the result, zero on entry.  d_bits null: one set, every point,
// its first step in known_start[0] — no bitmap exists and none is read.
idist_status grouped_device(const idist_index* idx, idist_search_ctx* ctx, const float* d_qk, uint32_t nq, const uint32_t* d_bits,
                            uint32_t n_sets, const uint32_t* d_setof, const uint32_t* set_of, const uint32_t* d_groups, uint32_t k,
                            int32_t max_rungs, AllowedOut o, uint32_t* d_ogroup, const uint32_t* known_start) {
    const uint32_t n = idx->n, words = (n + 31u) / 32u;
    auto grouped_out = [&](const AllowedOut& out) {
        return GroupedOut{out.pid, out.dist, d_ogroup, out.count, out.rung, out.counters, out.pending, k};
    };
    auto select_rung = [&](const AllowedOut& out, uint32_t ef, const uint32_t* d_list, uint32_t np, uint32_t r) {
        auto select_pass = [&]() -> idist_status {
            return launch_grouped_select(grouped_out(out), d_groups, n, d_bits, words, d_setof, ctx->d_pid, reinterpret_cast<const uint32_t*>(ctx->d_dist.p), ctx->d_cnt,
                                         out.counters ? ctx->d_ctr.p : nullptr, ef, d_list, np, r, kGroupedRung, ctx->stream);
        };
        return ladder_timed(ctx, 0, select_pass);
    };
    auto exact_step = [&](const AllowedOut& out, const uint32_t*& d_list, const float*& d_pq, uint32_t& np, auto& gather) {
        return grouped_exact_rounds(idx, ctx, grouped_out(out), d_groups, d_bits, d_setof, d_list, d_pq, np, gather);
    };
    return sets_ladder_device(idx, ctx, d_qk, nq, d_bits, n_sets, d_setof, set_of, k, max_rungs, o, select_rung, exact_step, known_start);
}

}  // namespace
}  // extern "C++"

// set_of == NULL: query q uses set q — the call's own_set, kept in *keep for its duration
static const uint32_t* set_of_or_identity(const uint32_t* set_of, uint32_t nq, std::vector<uint32_t>* keep) {
    if (set_of) return set_of;
    keep->resize(nq);
    for (uint32_t q = 0; q < nq; q++) (*keep)[q] = q;
    return keep->data();
}

// The several-sets call behind its argument checks, for sets from either source: stage, the call on the device, report, download.
// nq > 0; the trivial cases (n == 0, ef_search == 0) are answered here.
static idist_status allowed_sets_call(const idist_index* idx, idist_search_ctx* ctx, const float* queries, uint32_t nq, const SetsSource& src,
                                      uint32_t k, int32_t max_rungs, uint32_t* out_pid, float* out_dist, uint32_t* out_count,
                                      uint32_t* out_rung, uint32_t* out_counters) {
    const uint32_t n = idx->n;
    if (n == 0 || idx->cfg.ef_search == 0) {                                 // step 1: nothing to find, whatever the sets
        fill_nothing_found(nq, k, out_pid, out_dist, out_count, out_rung, out_counters);
        return IDIST_OK;
    }
    HIPCHK(hipSetDevice(idx->device));
    hipStream_t stream = ctx->stream;
    const MetricPasses metric(idx);
    AllowedOut o{};
    CHK(allowed_out_in_ctx(ctx, nq, k, out_counters != nullptr, &o));
    CHK(stage_sets(ctx, n, nq, src));
    const float* d_qk = nullptr;
    CHK(ladder_upload_queries(idx, ctx, metric, queries, nq, &d_qk));
    CHK(allowed_sets_device(idx, ctx, d_qk, nq, ctx->al_bits, src.n_sets, ctx->al_setof, src.set_of, k, max_rungs, o));
    CHK(metric.report(ctx->al_odist.as<float>(), ctx->d_sq, nq, k, stream));
    CHK(allowed_download(ctx, nq, k, out_pid, out_dist, out_count, out_rung, out_counters));
    HIPCHK(hipStreamSynchronize(stream));
    CHK(attr_time_resolve(ctx));
    return ladder_times_resolve(ctx);
}

idist_status idist_search_batch_allowed_sets(const idist_index* idx, idist_search_ctx* ctx, const float* queries, uint32_t nq,
                                             const uint32_t* allow_bits, uint32_t n_sets, const uint32_t* set_of, uint32_t k,
                                             int32_t max_rungs, uint32_t* out_pid, float* out_dist, uint32_t* out_count,
                                             uint32_t* out_rung, uint32_t* out_counters) {
    CHK(check_ctx(idx, ctx));
    CHK(check_ladder_args(max_rungs, k, idx->cfg.ef_search));
    CHK(check_sets_args(n_sets, set_of, nq));
    if (nq == 0) return IDIST_OK;
    if (!queries || !out_pid || !out_dist || !out_count || (idx->n && !allow_bits)) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    std::vector<uint32_t> identity;
    SetsSource src;
    src.bits = allow_bits; src.n_sets = n_sets; src.set_of = set_of_or_identity(set_of, nq, &identity);
    return allowed_sets_call(idx, ctx, queries, nq, src, k, max_rungs, out_pid, out_dist, out_count, out_rung, out_counters);
}

// ---- the attribute on the device and the calls that read it ----
static idist_status check_n_cols(uint32_t n_cols) {
    if (n_cols < 1 || n_cols > 64) return fail(IDIST_ERR_INVALID_ARG, "n_cols %u: a table has 1 to 64 columns", n_cols);
    return IDIST_OK;
}
// a slice's points [first, first + sl.n) of every column of values [n_cols][n_total] -> sl.v [n_cols][sl.n], on the slice's device
static idist_status attr_upload_slice(idist_attr::Slice& sl, const uint32_t* values, uint32_t n_cols, size_t n_total, size_t first) {
    if (!sl.n) return IDIST_OK;
    HIPCHK(hipSetDevice(sl.device));
    CHK(sl.v.grow((size_t)n_cols * sl.n * 4));
    if (n_cols == 1) HIPCHK(hipMemcpy(sl.v.p, values + first, (size_t)sl.n * 4, hipMemcpyHostToDevice));
    else HIPCHK(hipMemcpy2D(sl.v.p, (size_t)sl.n * 4, values + first, n_total * 4, (size_t)sl.n * 4, n_cols, hipMemcpyHostToDevice));
    return IDIST_OK;
}

idist_status idist_attr_new_columns(const idist_index* idx, const uint32_t* values, uint32_t n_cols, idist_attr** out) {
    if (!idx || !out) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    CHK(check_n_cols(n_cols));
    if (idx->n && !values) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    std::unique_ptr<idist_attr> a(new idist_attr());
    a->owner_uid = idx->uid;
    a->n_cols = n_cols;
    a->parts.resize(1);
    idist_attr::Slice& sl = a->parts[0];
    sl.n = idx->n;
    sl.device = idx->device;
    CHK(attr_upload_slice(sl, values, n_cols, sl.n, 0));
    *out = a.release();
    return IDIST_OK;
}
idist_status idist_attr_new(const idist_index* idx, const uint32_t* values, idist_attr** out) { return idist_attr_new_columns(idx, values, 1, out); }

idist_status idist_partitioned_attr_new_columns(const idist_partitioned* p, const uint32_t* values, uint32_t n_cols, idist_attr** out) {
    if (!p || !out) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    CHK(check_n_cols(n_cols));
    CHK(partitioned_check(const_cast<idist_partitioned*>(p), nullptr));
    const size_t P = p->parts.size();
    if (p->base[P] && !values) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    std::unique_ptr<idist_attr> a(new idist_attr());
    a->owner_uid = p->uid;
    a->partitioned = true;
    a->n_cols = n_cols;
    a->parts.resize(P);
    for (size_t i = 0; i < P; i++) {
        idist_attr::Slice& sl = a->parts[i];
        sl.n = p->parts[i].idx->n;
        sl.device = part_device(p, i);
        CHK(attr_upload_slice(sl, values, n_cols, p->base[P], p->base[i]));
    }
    *out = a.release();
    return IDIST_OK;
}
idist_status idist_partitioned_attr_new(const idist_partitioned* p, const uint32_t* values, idist_attr** out) {
    return idist_partitioned_attr_new_columns(p, values, 1, out);
}

void idist_attr_free(idist_attr* a) { delete a; }

idist_status idist_attr_bitmaps_device(const void* d_values, uint32_t n, const void* d_lo, const void* d_hi, uint32_t n_sets, void* d_out,
                                       int32_t device, void* hip_stream) {
    if (n == 0 || n_sets == 0) return IDIST_OK;
    if (!d_values || !d_lo || !d_hi || !d_out) return fail(IDIST_ERR_INVALID_ARG, "null device pointer");
    CHK(check_device(device));
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    return launch_attr_bitmaps((const uint32_t*)d_values, n, (const uint32_t*)d_lo, (const uint32_t*)d_hi, n_sets, (uint32_t*)d_out,
                               launch_cus(prop.multiProcessorCount), (hipStream_t)hip_stream);
}

idist_status idist_attr_match_bitmaps_device(const void* d_values, uint32_t n, uint32_t n_cols, uint64_t col_pitch, const void* d_clauses,
                                             const void* d_and_lims, const void* d_or_lims, uint32_t n_sets, void* d_out, int32_t device,
                                             void* hip_stream) {
    if (n == 0 || n_sets == 0) return IDIST_OK;
    if (!d_values || !d_and_lims || !d_or_lims || !d_out) return fail(IDIST_ERR_INVALID_ARG, "null device pointer");   // (d_clauses: a program may have none)
    CHK(check_n_cols(n_cols));
    if (col_pitch < n) return fail(IDIST_ERR_INVALID_ARG, "col_pitch %llu: a column holds n = %u values", (unsigned long long)col_pitch, n);
    CHK(check_device(device));
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    return launch_attr_match((const uint32_t*)d_values, n, n_cols, col_pitch, (const AttrClause*)d_clauses, (const uint32_t*)d_and_lims,
                             (const uint32_t*)d_or_lims, n_sets, (uint32_t*)d_out, launch_cus(prop.multiProcessorCount), (hipStream_t)hip_stream);
}

idist_status idist_search_batch_attr(const idist_index* idx, idist_search_ctx* ctx, const idist_attr* attr, const float* queries, uint32_t nq,
                                     const uint32_t* lo, const uint32_t* hi, uint32_t n_cond, uint32_t k, int32_t max_rungs,
                                     uint32_t* out_pid, float* out_dist, uint32_t* out_count, uint32_t* out_rung, uint32_t* out_counters) {
    CHK(check_ctx(idx, ctx));
    CHK(check_attr(attr, idx->uid, false));
    ctx->at_ms = 0.0f;
    CHK(check_ladder_args(max_rungs, k, idx->cfg.ef_search));
    CHK(check_cond_args(lo, hi, n_cond, nq));
    if (nq == 0) return IDIST_OK;
    if (!queries || !out_pid || !out_dist || !out_count) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    AttrConds g;
    attr_group(lo, hi, n_cond, nq, &g);
    return allowed_sets_call(idx, ctx, queries, nq, g.source(attr), k, max_rungs, out_pid, out_dist, out_count, out_rung, out_counters);
}

idist_status idist_search_batch_match(const idist_index* idx, idist_search_ctx* ctx, const idist_attr* attr, const float* queries, uint32_t nq,
                                      const idist_attr_conds* conds, uint32_t k, int32_t max_rungs, uint32_t* out_pid, float* out_dist,
                                      uint32_t* out_count, uint32_t* out_rung, uint32_t* out_counters) {
    CHK(check_ctx(idx, ctx));
    CHK(check_attr(attr, idx->uid, false));
    ctx->at_ms = 0.0f;
    CHK(check_ladder_args(max_rungs, k, idx->cfg.ef_search));
    CHK(check_match_args(conds, nq, attr->n_cols));
    if (nq == 0) return IDIST_OK;
    if (!queries || !out_pid || !out_dist || !out_count) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    MatchConds g;
    match_group(conds, conds->n_cond, nq, &g);
    return allowed_sets_call(idx, ctx, queries, nq, g.source(attr), k, max_rungs, out_pid, out_dist, out_count, out_rung, out_counters);
}

// ---- grouped search ----
idist_status idist_search_batch_grouped(const idist_index* idx, idist_search_ctx* ctx, const idist_attr* attr, uint32_t group_col,
                                        const float* queries, uint32_t nq, const idist_attr_conds* conds, uint32_t k, int32_t max_rungs,
                                        uint32_t* out_pid, float* out_dist, uint32_t* out_group, uint32_t* out_count, uint32_t* out_rung,
                                        uint32_t* out_counters) {
    CHK(check_ctx(idx, ctx));
    CHK(check_attr(attr, idx->uid, false));
    if (group_col >= attr->n_cols)
        return fail(IDIST_ERR_INVALID_ARG, "group_col %u, but the table has %u column%s", group_col, attr->n_cols, attr->n_cols == 1 ? "" : "s");
    ctx->at_ms = 0.0f;
    CHK(check_ladder_args(max_rungs, k, idx->cfg.ef_search));
    if (conds) CHK(check_match_args(conds, nq, attr->n_cols));
    if (nq == 0) return IDIST_OK;
    if (!queries || !out_pid || !out_dist || !out_count) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    const uint32_t n = idx->n;
    if (n == 0 || idx->cfg.ef_search == 0) {                                 // step 1: nothing to find
        fill_nothing_found(nq, k, out_pid, out_dist, out_count, out_rung, out_counters);
        if (out_group) memset(out_group, 0, (size_t)nq * k * 4);
        return IDIST_OK;
    }
    // A: the query's condition, grouped and staged as idist_search_batch_match does — or every point: one set that needs no bitmap
    // and no count, |A| = n being known (the start rule on the host: rung 0 when a rung is permitted and n > k, else exact)
    MatchConds g;
    std::vector<uint32_t> one_set;
    uint32_t first_step = kRungExact;
    if (conds) match_group(conds, conds->n_cond, nq, &g);
    else {
        one_set.assign(nq, 0u);
        if (n > k && make_ladder(idx->cfg.ef_search, max_rungs).n_rungs) first_step = 0u;   // (E[0] n >= k n: k <= ef_search was checked)
    }
    HIPCHK(hipSetDevice(idx->device));
    hipStream_t stream = ctx->stream;
    const MetricPasses metric(idx);
    const size_t ob = (size_t)nq * k * 4;
    AllowedOut o{};
    CHK(allowed_out_in_ctx(ctx, nq, k, out_counters != nullptr, &o));
    CHK(ctx->gr_ogroup.grow(ob));
    HIPCHK(hipMemsetAsync(ctx->gr_ogroup.p, 0, ob, stream));
    if (conds) {
        CHK(stage_sets(ctx, n, nq, g.source(attr)));
    } else {
        CHK(ctx->al_setof.grow((size_t)nq * 4));
        HIPCHK(hipMemsetAsync(ctx->al_setof.p, 0, (size_t)nq * 4, stream));
    }
    const float* d_qk = nullptr;
    CHK(ladder_upload_queries(idx, ctx, metric, queries, nq, &d_qk));
    CHK(grouped_device(idx, ctx, d_qk, nq, conds ? ctx->al_bits.p : nullptr, conds ? g.n_sets : 1u, ctx->al_setof,
                       conds ? g.set_of.data() : one_set.data(), attr->parts[0].v.p + (size_t)group_col * n, k, max_rungs, o, ctx->gr_ogroup,
                       conds ? nullptr : &first_step));
    CHK(metric.report(ctx->al_odist.as<float>(), ctx->d_sq, nq, k, stream));
    CHK(allowed_download(ctx, nq, k, out_pid, out_dist, out_count, out_rung, out_counters));
    if (out_group) HIPCHK(hipMemcpyAsync(out_group, ctx->gr_ogroup.p, ob, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    CHK(attr_time_resolve(ctx));
    return ladder_times_resolve(ctx);
}

idist_status idist_grouped_collapse_device(const void* d_pid, const void* d_dist, const void* d_count, uint32_t nq, uint32_t width,
                                           const void* d_groups, uint32_t n, const void* d_bits, uint32_t k, void* d_out_pid,
                                           void* d_out_dist, void* d_out_group, void* d_out_count, int32_t device, void* hip_stream) {
    if (k == 0 || k > IDIST_MAX_EF) return fail(IDIST_ERR_INVALID_ARG, "k %u out of [1,%u]", k, IDIST_MAX_EF);
    if (nq == 0) return IDIST_OK;
    if (!d_count || !d_out_pid || !d_out_dist || !d_out_group || !d_out_count || (width && (!d_pid || !d_dist)) || (n && !d_groups))
        return fail(IDIST_ERR_INVALID_ARG, "null device pointer");
    CHK(check_device(device));
    HIPCHK(hipSetDevice(device));
    const GroupedOut g{(uint32_t*)d_out_pid, (uint32_t*)d_out_dist, (uint32_t*)d_out_group, (uint32_t*)d_out_count, nullptr, nullptr, nullptr, k};
    return launch_grouped_select(g, (const uint32_t*)d_groups, n, (const uint32_t*)d_bits, (n + 31u) / 32u, nullptr, (const uint32_t*)d_pid,
                                 (const uint32_t*)d_dist, (const uint32_t*)d_count, nullptr, width, nullptr, nq, 0u, kGroupedWhole,
                                 (hipStream_t)hip_stream);
}

idist_status idist_search_ctx_attr_bitmap_ms(idist_search_ctx* ctx, float* ms) {
    if (!ctx || !ms) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    *ms = ctx->at_ms;
    return IDIST_OK;
}

idist_status idist_allowed_slice_device(const void* d_bits, uint32_t n_sets, uint32_t pitch_words, uint64_t bit_offset, uint32_t n_out,
                                        void* d_out, int32_t device, void* hip_stream) {
    if (n_out == 0 || n_sets == 0) return IDIST_OK;
    if (!d_bits || !d_out) return fail(IDIST_ERR_INVALID_ARG, "null device pointer");
    const uint64_t w_end = (bit_offset + n_out + 31u) / 32u;             // words of a source row that may be read
    if (pitch_words < w_end)
        return fail(IDIST_ERR_INVALID_ARG, "pitch_words %u: bits [%llu, %llu) of a row need %llu words", pitch_words,
                    (unsigned long long)bit_offset, (unsigned long long)(bit_offset + n_out), (unsigned long long)w_end);
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) return fail(IDIST_ERR_NO_DEVICE, "no HIP device visible; libidist has no CPU path");
    if (device < 0 || device >= cnt) return fail(IDIST_ERR_INVALID_ARG, "device %d out of range [0,%d)", device, cnt);
    HIPCHK(hipSetDevice(device));
    const size_t total = (size_t)n_sets * (((size_t)n_out + 31u) / 32u);
    const uint32_t grid = (uint32_t)std::min<size_t>((total + 255u) / 256u, 4096u);   // one lane per output word; the kernel strides over the rest
    IDIST_LAUNCH(allowed_slice_kernel, grid, 256, 0, (hipStream_t)hip_stream, (const uint32_t*)d_bits, n_sets, pitch_words, bit_offset, n_out,
                 (uint32_t*)d_out);
    HIPCHK(hipGetLastError());
    return IDIST_OK;
}

// The sets of a restricted call over the parts (the sets name GLOBAL ids), every part's in its context's al_bits, its device's
// Dev::d_setof filled.  N > 0, nq > 0.
//   1. the set of every query, once per distinct device that has something to search;
//   2. the caller's bitmaps: the words [base / 32, ceil((base + n_p) / 32)) of every set in ONE strided copy out of the caller's
//      buffer (which is only read), then the slice kernel shifts them by base % 32 on the part's stream — the part's own
//      [n_sets][(n_p + 31) / 32], the bits behind n_p cleared.  p->al_slice_ms: the host time of it;
//      an attribute: every part makes its bitmaps from ITS slice of the values with attr_bitmaps_kernel on its own stream — no
//      upload of n bits, no slice kernel, and by construction the slice of the global bitmap.  p->al_slice_ms comes from the
//      parts' events once their streams have been synchronised (partitioned_attr_times).
static idist_status partitioned_stage_sets(idist_partitioned* p, uint32_t nq, const SetsSource& src) {
    const size_t P = p->parts.size();
    const size_t W = ((size_t)p->base[P] + 31u) / 32u;
    const uint32_t n_sets = src.n_sets;
    CHK(for_each_used_device(p, [&](idist_partitioned::Dev& dv) -> idist_status {
        CHK(dv.d_setof.grow((size_t)nq * 4));
        HIPCHK(hipMemcpy(dv.d_setof, src.set_of, (size_t)nq * 4, hipMemcpyHostToDevice));
        return IDIST_OK;
    }));
    if (src.attr) {
        for (size_t i = 0; i < P; i++) {
            idist_partitioned::Part& pt = p->parts[i];
            if (!pt.ctx) continue;
            HIPCHK(hipSetDevice(p->devs[pt.dev_slot].device));
            pt.ctx->at_ms = 0.0f;
            CHK(attr_stage_bitmaps(pt.ctx, src.attr->parts[i].v, pt.idx->n, src));
        }
        return IDIST_OK;
    }
    const uint32_t* allow_bits = src.bits;
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t i = 0; i < P; i++) {
        idist_partitioned::Part& pt = p->parts[i];
        if (!pt.ctx) continue;
        const uint32_t n_p = pt.idx->n, w0 = p->base[i] / 32u, sh = p->base[i] % 32u;
        const size_t nw = ((size_t)sh + n_p + 31u) / 32u, words = ((size_t)n_p + 31u) / 32u;
        HIPCHK(hipSetDevice(p->devs[pt.dev_slot].device));
        CHK(pt.ctx->al_raw.grow((size_t)n_sets * nw * 4));
        CHK(pt.ctx->al_bits.grow((size_t)n_sets * words * 4));
        if (n_sets == 1) HIPCHK(hipMemcpy(pt.ctx->al_raw.p, allow_bits + w0, nw * 4, hipMemcpyHostToDevice));
        else HIPCHK(hipMemcpy2D(pt.ctx->al_raw.p, nw * 4, allow_bits + w0, W * 4, nw * 4, n_sets, hipMemcpyHostToDevice));
        const size_t total = (size_t)n_sets * words;
        const uint32_t grid = (uint32_t)std::min<size_t>((total + 255u) / 256u, (size_t)std::max(pt.ctx->n_cu, 1) * 8u);
        const uint32_t* raw = pt.ctx->al_raw;
        uint32_t* bits = pt.ctx->al_bits;
        IDIST_LAUNCH(allowed_slice_kernel, grid, 256, 0, pt.ctx->stream, raw, n_sets, (uint32_t)nw, (uint64_t)sh, n_p, bits);
        HIPCHK(hipGetLastError());
    }
    for (size_t i = 0; i < P; i++) {                     // (waited for only to be timed: the ladders run on the same streams)
        idist_partitioned::Part& pt = p->parts[i];
        if (!pt.ctx || !pt.ctx->knobs.events) continue;
        HIPCHK(hipSetDevice(p->devs[pt.dev_slot].device));
        HIPCHK(hipStreamSynchronize(pt.ctx->stream));
    }
    p->al_slice_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return IDIST_OK;
}
// an attribute call, after the parts' streams have been synchronised: the parts' bitmap kernels, summed
static void partitioned_attr_times(idist_partitioned* p, const SetsSource& src) {
    if (!src.attr) return;
    p->al_slice_ms = 0.0f;
    for (auto& pt : p->parts)
        if (pt.ctx) p->al_slice_ms += pt.ctx->at_ms;
}

// an attribute of a partitioned call: made for p, and the parts are still the sizes its slices were cut for (partitioned_check ran)
static idist_status check_partitioned_attr(const idist_partitioned* p, const idist_attr* attr) {
    CHK(check_attr(attr, p->uid, true));
    for (size_t i = 0; i < p->parts.size(); i++)
        if (attr->parts.size() != p->parts.size() || attr->parts[i].n != p->parts[i].idx->n)
            return fail(IDIST_ERR_INVALID_ARG, "attr does not belong to this partitioned index");
    return IDIST_OK;
}

// The restricted search over the parts behind its argument checks, for sets from either source.  nq > 0.
static idist_status partitioned_allowed_sets_call(idist_partitioned* p, uint32_t ef, const float* queries, uint32_t nq, const SetsSource& src,
                                                  uint32_t k, int32_t max_rungs, uint32_t* out_pid, float* out_dist, uint32_t* out_count,
                                                  uint32_t* out_rung, uint32_t* out_counters) {
    const size_t P = p->parts.size();
    const uint32_t N = p->base[P], n_sets = src.n_sets;
    const uint32_t* set_of = src.set_of;
    if (out_rung) std::fill(out_rung, out_rung + (size_t)nq * P, (uint32_t)IDIST_RUNG_NONE);   // (empty parts keep it)
    p->al_slice_ms = 0.0f;
    if (N == 0 || ef == 0) {                                                 // nothing to find, whatever the sets
        fill_nothing_found(nq, k, out_pid, out_dist, out_count, nullptr, out_counters);     // (out_rung [nq][P] is filled above)
        return IDIST_OK;
    }
    const bool counters = out_counters != nullptr;
    const size_t row = (size_t)nq * k;
    HIPCHK(hipSetDevice(p->merge_device));
    CHK(partitioned_reserve(p, nq, k, k));
    CHK(p->s_rung.grow(P * nq * 4));
    CHK(partitioned_prepare_report(p, queries, nq));
    // 1. the queries and the set of every query, once per distinct device that has something to search; 2. every part's bitmaps
    CHK(partitioned_upload_queries(p, queries, nq));
    CHK(partitioned_stage_sets(p, nq, src));
    // 3. the ladders block on the host, one synchronisation per rung: one thread per non-empty part, each with the part's own context
    //    and stream.  On the merge device straight into the part's slice of the staging memory, elsewhere into memory of the part's
    //    device followed by one peer copy per array (partitioned_fan_out, partitioned_send).
    CHK(partitioned_fan_out(p, [&](size_t i) -> idist_status {
        idist_partitioned::Part& pt = p->parts[i];
        idist_search_ctx* ctx = pt.ctx;
        const idist_partitioned::Dev& dv = p->devs[pt.dev_slot];
        const int32_t dev = dv.device;
        uint32_t *s_pid = p->s_pid + i * row, *s_cnt = p->s_cnt + i * nq, *s_ctr = p->s_ctr + i * nq * 3, *s_rung = p->s_rung + i * nq;
        float* s_dist = p->s_dist + i * row;
        HIPCHK(hipSetDevice(dev));
        AllowedOut o{};
        if (dev == p->merge_device) {
            o.pid = s_pid; o.dist = reinterpret_cast<uint32_t*>(s_dist); o.count = s_cnt; o.rung = s_rung; o.counters = counters ? s_ctr : nullptr;
        } else {
            CHK(allowed_out_in_ctx(ctx, nq, k, counters, &o));
        }
        CHK(allowed_sets_device(pt.idx, ctx, dv.d_q, nq, ctx->al_bits, n_sets, dv.d_setof, set_of, k, max_rungs, o));
        if (dev != p->merge_device) CHK(partitioned_send(p, i, nq, k, o.pid, o.dist, o.count, o.rung, counters ? o.counters : nullptr));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        CHK(attr_time_resolve(ctx));
        return ladder_times_resolve(ctx);
    }));
    partitioned_attr_times(p, src);
    // 4. the union: empty parts hand in lists of length 0; the parts' rungs come back [P][nq] and are transposed on the host
    HIPCHK(hipSetDevice(p->merge_device));
    CHK(partitioned_zero_empty_parts(p, nq, counters));
    std::vector<uint32_t> rungs;
    if (out_rung) {
        rungs.resize(P * nq);
        HIPCHK(hipMemcpyAsync(rungs.data(), p->s_rung, P * nq * 4, hipMemcpyDeviceToHost, p->stream));
    }
    CHK(partitioned_merge(p, nq, k, k, counters, out_pid, out_dist, out_count, out_counters));
    partitioned_transpose_rungs(p, rungs, nq, out_rung);
    return IDIST_OK;
}

idist_status idist_partitioned_search_batch_allowed_sets(idist_partitioned* p, const float* queries, uint32_t nq,
                                                         const uint32_t* allow_bits, uint32_t n_sets, const uint32_t* set_of, uint32_t k,
                                                         int32_t max_rungs, uint32_t* out_pid, float* out_dist, uint32_t* out_count,
                                                         uint32_t* out_rung, uint32_t* out_counters) {
    if (!p) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    uint32_t ef = 0;
    CHK(partitioned_check(p, &ef));
    CHK(check_ladder_args(max_rungs, k, ef));
    CHK(check_sets_args(n_sets, set_of, nq));
    if (nq == 0) return IDIST_OK;
    if (!queries || !out_pid || !out_dist || !out_count || (p->base[p->parts.size()] && !allow_bits)) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    std::vector<uint32_t> identity;
    SetsSource src;
    src.bits = allow_bits; src.n_sets = n_sets; src.set_of = set_of_or_identity(set_of, nq, &identity);
    return partitioned_allowed_sets_call(p, ef, queries, nq, src, k, max_rungs, out_pid, out_dist, out_count, out_rung, out_counters);
}

idist_status idist_partitioned_search_batch_attr(idist_partitioned* p, const idist_attr* attr, const float* queries, uint32_t nq,
                                                 const uint32_t* lo, const uint32_t* hi, uint32_t n_cond, uint32_t k, int32_t max_rungs,
                                                 uint32_t* out_pid, float* out_dist, uint32_t* out_count, uint32_t* out_rung,
                                                 uint32_t* out_counters) {
    if (!p) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    uint32_t ef = 0;
    CHK(partitioned_check(p, &ef));
    CHK(check_partitioned_attr(p, attr));
    CHK(check_ladder_args(max_rungs, k, ef));
    CHK(check_cond_args(lo, hi, n_cond, nq));
    if (nq == 0) return IDIST_OK;
    if (!queries || !out_pid || !out_dist || !out_count) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    AttrConds g;
    attr_group(lo, hi, n_cond, nq, &g);
    return partitioned_allowed_sets_call(p, ef, queries, nq, g.source(attr), k, max_rungs, out_pid, out_dist, out_count, out_rung, out_counters);
}

idist_status idist_partitioned_search_batch_match(idist_partitioned* p, const idist_attr* attr, const float* queries, uint32_t nq,
                                                  const idist_attr_conds* conds, uint32_t k, int32_t max_rungs, uint32_t* out_pid,
                                                  float* out_dist, uint32_t* out_count, uint32_t* out_rung, uint32_t* out_counters) {
    if (!p) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    uint32_t ef = 0;
    CHK(partitioned_check(p, &ef));
    CHK(check_partitioned_attr(p, attr));
    CHK(check_ladder_args(max_rungs, k, ef));
    CHK(check_match_args(conds, nq, attr->n_cols));
    if (nq == 0) return IDIST_OK;
    if (!queries || !out_pid || !out_dist || !out_count) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    MatchConds g;
    match_group(conds, conds->n_cond, nq, &g);
    return partitioned_allowed_sets_call(p, ef, queries, nq, g.source(attr), k, max_rungs, out_pid, out_dist, out_count, out_rung, out_counters);
}

idist_status idist_partitioned_last_allowed_slice_ms(idist_partitioned* p, float* ms) {
    if (!p || !ms) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    *ms = p->al_slice_ms;
    return IDIST_OK;
}

idist_status idist_search_ctx_allowed_kernel_ms(idist_search_ctx* ctx, float* select_ms, float* pending_ms, float* exact_ms) {
    if (!ctx || !select_ms || !pending_ms || !exact_ms) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    *select_ms = ctx->al_ms[0];
    *pending_ms = ctx->al_ms[1];
    *exact_ms = ctx->al_ms[2];
    return IDIST_OK;
}

// ---- range search: every point within a radius; the ef ladder over Hnsw::search, exact scan of every row ----
extern "C++" {
namespace {

// the result buffer keeps what it holds when it grows (DevBuf::grow alone frees first)
idist_status range_grow_keys(idist_search_ctx* ctx, uint64_t used, uint64_t need) {
    const size_t need_b = (size_t)need * 8;
    if (need_b <= ctx->rg_keys.cap) return IDIST_OK;
    DevBuf<uint64_t> fresh;
    CHK(fresh.grow(doubled_from(4096, need_b)));
    if (used) HIPCHK(hipMemcpyAsync(fresh, ctx->rg_keys, (size_t)used * 8, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->rg_keys = std::move(fresh);                     // (a swap: the old buffer leaves with `fresh`)
    return IDIST_OK;
}

// off [N + 1] = base + the exclusive prefix sum of cnt [N] (off[N]: the total), enqueued on the context's stream
// (chunk_sum: ceil(N / 64) u64 of scratch on the stream's device)
idist_status range_prefix_on(hipStream_t stream, uint64_t* chunk_sum, const uint32_t* cnt, uint64_t N, uint64_t base, uint64_t* off) {
    const uint64_t chunks = (N + 63u) / 64u;
    if (chunks == 0) return IDIST_OK;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(chunks, 65536u);
    IDIST_LAUNCH(range_chunk_sums_kernel, grid, 64, 0, stream, cnt, N, chunk_sum);
    IDIST_LAUNCH(range_offsets_kernel, grid, 64, 0, stream, cnt, N, chunk_sum, base, off);
    HIPCHK(hipGetLastError());
    return IDIST_OK;
}
idist_status range_prefix(idist_search_ctx* ctx, const uint32_t* cnt, uint64_t N, uint64_t base, uint64_t* off) {
    const uint64_t chunks = (N + 63u) / 64u;
    if (chunks == 0) return IDIST_OK;
    CHK(ctx->rg_chunks.grow(doubled_from(256, (size_t)chunks * 8)));
    return range_prefix_on(ctx->stream, ctx->rg_chunks, cnt, N, base, off);
}

// every list [ex_off[p], + ex_len[p]) of the result buffer ascending; max_len: the longest of them
idist_status range_sort(idist_search_ctx* ctx, uint32_t np, uint64_t max_len) {
    if (max_len < 2) return IDIST_OK;
    uint64_t P = 2;
    while (P < max_len) P <<= 1;
    const uint32_t chunk = ctx->knobs.range_sort_chunk ? ctx->knobs.range_sort_chunk : 2048u;
    const uint32_t chunks_max = (uint32_t)std::max<uint64_t>(P / chunk, 1u);
    const uint64_t pairs_max = P / 2u;
    uint64_t* keys = ctx->rg_keys;
    const uint64_t* off = ctx->rg_exoff;
    const uint32_t* len = ctx->rg_exlen;
    const uint64_t cap = (uint64_t)std::max(ctx->n_cu, 1) * 64u;
    const uint32_t grid_l = (uint32_t)std::min<uint64_t>((uint64_t)np * chunks_max, cap);
    const uint32_t grid_g = (uint32_t)std::min<uint64_t>((uint64_t)np * ((pairs_max + 63u) / 64u), cap);
    const size_t smem = (size_t)chunk * 8;
    IDIST_LAUNCH(range_sort_kernel, grid_l, 64, smem, ctx->stream, keys, off, len, np, chunk, chunks_max, pairs_max, (uint32_t)kSortLocal,
                 (uint64_t)0, (uint64_t)0);
    for (uint64_t k = 2ull * chunk; k <= P; k <<= 1) {
        IDIST_LAUNCH(range_sort_kernel, grid_g, 64, 0, ctx->stream, keys, off, len, np, chunk, chunks_max, pairs_max, (uint32_t)kSortFlip, k,
                     (uint64_t)0);
        for (uint64_t j = k / 4u; j >= chunk; j >>= 1)
            IDIST_LAUNCH(range_sort_kernel, grid_g, 64, 0, ctx->stream, keys, off, len, np, chunk, chunks_max, pairs_max,
                         (uint32_t)kSortDisperse, k, j);
        IDIST_LAUNCH(range_sort_kernel, grid_l, 64, smem, ctx->stream, keys, off, len, np, chunk, chunks_max, pairs_max,
                     (uint32_t)kSortLocalTail, k, (uint64_t)0);
    }
    HIPCHK(hipGetLastError());
    return IDIST_OK;
}

idist_status range_too_many(uint64_t known, uint64_t max_total, const char* after) {
    return fail(IDIST_ERR_INVALID_ARG, "range search: %llu results known after %s exceed max_total %llu (nothing is returned)",
                (unsigned long long)known, after, (unsigned long long)max_total);
}

// the argument checks of a range call, each message once (the single index and the partitioned one)
idist_status check_range_args(const float* queries, uint32_t nq, const float* radius, uint32_t n_radius, int32_t max_rungs,
                              const uint64_t* out_lims) {
    CHK(check_max_rungs(max_rungs));
    if (!out_lims) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    if (nq && n_radius != 1 && n_radius != nq) return fail(IDIST_ERR_INVALID_ARG, "n_radius %u: 1 (one radius for the batch) or nq = %u", n_radius, nq);
    if (nq && (!queries || !radius)) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    for (uint32_t i = 0; nq && i < n_radius; i++)
        if (radius[i] != radius[i]) {
            if (n_radius == 1) return fail(IDIST_ERR_INVALID_ARG, "the radius of the batch (query 0 and every other) is NaN");
            return fail(IDIST_ERR_INVALID_ARG, "the radius of query %u is NaN", i);
        }
    return IDIST_OK;
}

// a range call begins: the context holds nothing, times nothing
void range_begin(const idist_index* idx, idist_search_ctx* ctx, uint32_t nq) {
    ctx->rg_valid = false;
    ctx->rg_nq = nq;
    ctx->rg_total = 0;
    ctx->rg_metric = idx->cfg.metric;
    ctx->al_ms[3] = ctx->al_ms[4] = ctx->al_ms[5] = 0.0f;
    ctx->al_ev_used = 0;
}

// the allowed sets of a restricted range search, on the device: bits [n_sets][words], set_of [nq]
struct RangeSets {
    const uint32_t* bits;
    const uint32_t* set_of;
    uint32_t n_sets, words;
};

idist_status range_search_device(const idist_index* idx, idist_search_ctx* ctx, const float* d_qk, const float* d_sq, uint32_t nq,
                                 const float* radius, uint32_t n_radius, int32_t max_rungs, uint64_t max_total, bool counters,
                                 uint64_t* total_out, const RangeSets* sets = nullptr);
idist_status range_finish(idist_search_ctx* ctx, uint32_t nq, uint64_t total, uint64_t* out_lims, uint32_t* out_rung, uint32_t* out_counters);

}  // namespace
}  // extern "C++"

idist_status idist_search_batch_range(const idist_index* idx, idist_search_ctx* ctx, const float* queries, uint32_t nq,
                                      const float* radius, uint32_t n_radius, int32_t max_rungs, uint64_t max_total,
                                      uint64_t* out_lims, uint32_t* out_rung, uint32_t* out_counters) {
    CHK(check_ctx(idx, ctx));
    ctx->rg_valid = false;                                                   // whatever happens next, the previous results are gone
    CHK(check_range_args(queries, nq, radius, n_radius, max_rungs, out_lims));
    range_begin(idx, ctx, nq);
    if (nq == 0 || idx->n == 0 || idx->cfg.ef_search == 0) {                 // step 1: nothing to find
        std::fill(out_lims, out_lims + nq + 1, (uint64_t)0);
        fill_nothing_found(nq, 0, nullptr, nullptr, nullptr, out_rung, out_counters);
        ctx->rg_valid = true;
        return IDIST_OK;
    }
    HIPCHK(hipSetDevice(idx->device));
    const bool counters = out_counters != nullptr;
    const float* d_qk = nullptr;                                 // (the metric's report is applied once, to what the fetch hands out)
    CHK(ladder_upload_queries(idx, ctx, MetricPasses(idx), queries, nq, &d_qk));
    uint64_t total = 0;
    CHK(range_search_device(idx, ctx, d_qk, ctx->d_sq, nq, radius, n_radius, max_rungs, max_total, counters, &total));
    return range_finish(ctx, nq, total, out_lims, out_rung, out_counters);
}

// ---- restricted range search: every point of a query's own allowed set within its radius ----
// The call behind its argument checks, for sets from either source.  The previous results are gone already.
static idist_status range_allowed_sets_call(const idist_index* idx, idist_search_ctx* ctx, const float* queries, uint32_t nq, const float* radius,
                                            uint32_t n_radius, const SetsSource& src, int32_t max_rungs, uint64_t max_total, uint64_t* out_lims,
                                            uint32_t* out_rung, uint32_t* out_counters) {
    const uint32_t n = idx->n;
    range_begin(idx, ctx, nq);
    if (nq == 0 || n == 0 || idx->cfg.ef_search == 0) {                      // step 1: nothing to find, whatever the sets
        std::fill(out_lims, out_lims + nq + 1, (uint64_t)0);
        fill_nothing_found(nq, 0, nullptr, nullptr, nullptr, out_rung, out_counters);
        ctx->rg_valid = true;
        return IDIST_OK;
    }
    HIPCHK(hipSetDevice(idx->device));
    // the bitmaps and set_of as idist_search_batch_allowed_sets stages them
    CHK(stage_sets(ctx, n, nq, src));
    const float* d_qk = nullptr;
    CHK(ladder_upload_queries(idx, ctx, MetricPasses(idx), queries, nq, &d_qk));
    const RangeSets sets{ctx->al_bits, ctx->al_setof, src.n_sets, (n + 31u) / 32u};
    uint64_t total = 0;
    CHK(range_search_device(idx, ctx, d_qk, ctx->d_sq, nq, radius, n_radius, max_rungs, max_total, out_counters != nullptr, &total, &sets));
    CHK(range_finish(ctx, nq, total, out_lims, out_rung, out_counters));
    return attr_time_resolve(ctx);
}

idist_status idist_search_batch_range_allowed_sets(const idist_index* idx, idist_search_ctx* ctx, const float* queries, uint32_t nq,
                                                   const float* radius, uint32_t n_radius, const uint32_t* allow_bits, uint32_t n_sets,
                                                   const uint32_t* set_of, int32_t max_rungs, uint64_t max_total, uint64_t* out_lims,
                                                   uint32_t* out_rung, uint32_t* out_counters) {
    CHK(check_ctx(idx, ctx));
    ctx->rg_valid = false;                                                   // whatever happens next, the previous results are gone
    CHK(check_range_args(queries, nq, radius, n_radius, max_rungs, out_lims));
    CHK(check_sets_args(n_sets, set_of, nq));
    if (nq && idx->n && !allow_bits) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    std::vector<uint32_t> identity;
    SetsSource src;
    src.bits = allow_bits; src.n_sets = n_sets; src.set_of = set_of_or_identity(set_of, nq, &identity);
    return range_allowed_sets_call(idx, ctx, queries, nq, radius, n_radius, src, max_rungs, max_total, out_lims, out_rung, out_counters);
}

idist_status idist_search_batch_range_attr(const idist_index* idx, idist_search_ctx* ctx, const idist_attr* attr, const float* queries, uint32_t nq,
                                           const float* radius, uint32_t n_radius, const uint32_t* lo, const uint32_t* hi, uint32_t n_cond,
                                           int32_t max_rungs, uint64_t max_total, uint64_t* out_lims, uint32_t* out_rung, uint32_t* out_counters) {
    CHK(check_ctx(idx, ctx));
    ctx->rg_valid = false;                                                   // whatever happens next, the previous results are gone
    CHK(check_attr(attr, idx->uid, false));
    ctx->at_ms = 0.0f;
    CHK(check_range_args(queries, nq, radius, n_radius, max_rungs, out_lims));
    CHK(check_cond_args(lo, hi, n_cond, nq));
    AttrConds g;
    attr_group(lo, hi, nq ? n_cond : 0u, nq, &g);
    return range_allowed_sets_call(idx, ctx, queries, nq, radius, n_radius, g.source(attr), max_rungs, max_total, out_lims, out_rung, out_counters);
}

idist_status idist_search_batch_range_match(const idist_index* idx, idist_search_ctx* ctx, const idist_attr* attr, const float* queries, uint32_t nq,
                                            const float* radius, uint32_t n_radius, const idist_attr_conds* conds, int32_t max_rungs,
                                            uint64_t max_total, uint64_t* out_lims, uint32_t* out_rung, uint32_t* out_counters) {
    CHK(check_ctx(idx, ctx));
    ctx->rg_valid = false;                                                   // whatever happens next, the previous results are gone
    CHK(check_attr(attr, idx->uid, false));
    ctx->at_ms = 0.0f;
    CHK(check_range_args(queries, nq, radius, n_radius, max_rungs, out_lims));
    CHK(check_match_args(conds, nq, attr->n_cols));
    MatchConds g;
    match_group(conds, nq ? conds->n_cond : 0u, nq, &g);
    return range_allowed_sets_call(idx, ctx, queries, nq, radius, n_radius, g.source(attr), max_rungs, max_total, out_lims, out_rung, out_counters);
}

extern "C++" {
namespace {

// The end of a range call on one index: lims, the prefix sum of the counts in query order, with the rungs and counters on their way
// back to the caller; the call's last synchronisation; the context holds the results from here on.
idist_status range_finish(idist_search_ctx* ctx, uint32_t nq, uint64_t total, uint64_t* out_lims, uint32_t* out_rung, uint32_t* out_counters) {
    hipStream_t stream = ctx->stream;
    CHK(ctx->rg_lims.grow(((size_t)nq + 1) * 8));
    uint64_t* d_lims = ctx->rg_lims;
    auto lims_pass = [&]() -> idist_status { return range_prefix(ctx, ctx->rg_cnt, nq, 0, d_lims); };
    CHK(ladder_timed(ctx, 3, lims_pass));
    HIPCHK(hipMemcpyAsync(out_lims, d_lims, ((size_t)nq + 1) * 8, hipMemcpyDeviceToHost, stream));
    if (out_rung) HIPCHK(hipMemcpyAsync(out_rung, ctx->al_orung.p, (size_t)nq * 4, hipMemcpyDeviceToHost, stream));
    if (out_counters) HIPCHK(hipMemcpyAsync(out_counters, ctx->al_octr.p, (size_t)nq * 12, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    CHK(ladder_times_resolve(ctx));
    if (out_lims[nq] != total) return fail(IDIST_ERR_INTERNAL, "range search: the counts sum to %llu, the result buffer holds %llu",
                                           (unsigned long long)out_lims[nq], (unsigned long long)total);
    ctx->rg_total = total;
    ctx->rg_valid = true;
    return IDIST_OK;
}

// The search itself, for queries that are on the index's device already (d_qk [nq][kdim] as the kernels read them, d_sq: s(q) of a
// DOT index): the ladder and the exact step of DESIGN.md §4.9 on the context's stream, which is the current device's.  Afterwards
// the context holds the keys in completion order (rg_keys), every query's offset, count and report term (rg_off, rg_cnt, rg_term),
// its rung and counters (al_orung, al_octr); *total_out keys in all.  n > 0, ef_search > 0, nq > 0; range_begin has run.  The kernels
// enqueued last may still be running when this returns.
// sets != nullptr: the restricted range search of §4.10 — the same schedule with the bitmap in the select and copy passes and in the
// exact scan, a count pass in front, and pending lists that know every query's last rung: a query is gathered for rung r iff it is
// pending and r < last[q], so the batch is gathered once before rung 0 (a small set skips the ladder) and once more, whole, before
// the exact step.  sets == nullptr launches exactly what the plain call always launched.
idist_status range_search_device(const idist_index* idx, idist_search_ctx* ctx, const float* d_qk, const float* d_sq, uint32_t nq,
                                 const float* radius, uint32_t n_radius, int32_t max_rungs, uint64_t max_total, bool counters,
                                 uint64_t* total_out, const RangeSets* sets) {
    const uint32_t n = idx->n;
    const AllowedLadder lad = make_ladder(idx->cfg.ef_search, max_rungs);
    hipStream_t stream = ctx->stream;
    const uint32_t kdim = idx->kdim, kmetric = (uint32_t)idx->cfg.metric;
    CHK(ctx->rg_radius.grow((size_t)n_radius * 4));
    CHK(ctx->rg_lim.grow((size_t)nq * 8));
    CHK(ctx->rg_term.grow((size_t)nq * 4));
    CHK(ctx->rg_cnt.grow((size_t)nq * 4));
    CHK(ctx->rg_off.grow((size_t)nq * 8));
    CHK(ctx->rg_stepcnt.grow((size_t)nq * 4));
    CHK(ctx->rg_stepoff.grow(((size_t)nq + 1) * 8));
    CHK(ctx->al_flag.grow((size_t)nq * 4));
    CHK(ctx->al_list.grow((size_t)nq * 4));
    CHK(ctx->al_npend.grow(256));
    CHK(ctx->al_pq.grow((size_t)nq * kdim * 4));
    CHK(ctx->rg_list.grow((size_t)nq * 4));
    CHK(ctx->al_orung.grow((size_t)nq * 4));
    CHK(ctx->al_octr.grow((size_t)nq * 12));
    HIPCHK(hipMemcpyAsync(ctx->rg_radius.p, radius, (size_t)n_radius * 4, hipMemcpyHostToDevice, stream));
    RangeState st{};
    st.lim = ctx->rg_lim; st.term = ctx->rg_term; st.count = ctx->rg_cnt;
    st.off = ctx->rg_off; st.rung = ctx->al_orung; st.counters = counters ? ctx->al_octr.p : nullptr;
    st.pending = ctx->al_flag; st.nq = nq;
    const uint32_t waves_cap = (uint32_t)std::max(ctx->n_cu, 1) * 64u;
    auto init_pass = [&]() -> idist_status {
        const uint32_t grid = std::min<uint32_t>((nq + 255u) / 256u, (uint32_t)std::max(ctx->n_cu, 1) * 8u);
        IDIST_LAUNCH(range_init_kernel, grid, 256, 0, stream, st, ctx->rg_radius, n_radius, kmetric, d_sq, idx->dot_S);
        HIPCHK(hipGetLastError());
        return IDIST_OK;
    };
    CHK(ladder_timed(ctx, 3, init_pass));
    uint32_t np = nq;
    uint64_t total = 0;                                          // keys in the result buffer so far
    const uint32_t* d_list = nullptr;
    const float* d_pq = d_qk;
    uint32_t* step_cnt = ctx->rg_stepcnt;
    uint64_t* step_off = ctx->rg_stepoff;
    const uint32_t* d_last = nullptr;                            // restricted: the rungs query q may run are r < last[q]
    const uint32_t *s_bits = sets ? sets->bits : nullptr, *s_setof = sets ? sets->set_of : nullptr;
    const uint32_t s_words = sets ? sets->words : 0u, n_sets = sets ? sets->n_sets : 0u;
    // restricted: the queries of rung `rung` (d_last) or everything still pending (nullptr) into al_list / al_pq, their number read back
    auto gather = [&](uint32_t rung, const uint32_t* last) -> idist_status {
        CHK(ladder_pending(ctx, st.pending, nq, d_qk, kdim, ctx->al_list, 3, nullptr, rung, last));
        HIPCHK(hipMemcpyAsync(&np, ctx->al_npend.p, 4, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        d_list = ctx->al_list;
        d_pq = ctx->al_pq;
        return IDIST_OK;
    };
    if (sets) {
        CHK(ctx->al_size.grow((size_t)n_sets * 4));
        CHK(ctx->al_start.grow((size_t)n_sets * 4));
        CHK(ctx->al_first.grow((size_t)nq * 4));
        d_last = ctx->al_first;
        auto count_pass = [&]() -> idist_status {
            const uint32_t grid_c = std::min<uint32_t>(n_sets, (uint32_t)std::max(ctx->n_cu, 1) * 32u);
            IDIST_LAUNCH(range_allowed_count_kernel, grid_c, 64, 0, stream, s_bits, n, s_words, n_sets, lad,
                         ctx->al_size, ctx->al_start);
            const uint32_t grid_i = std::min<uint32_t>((nq + 255u) / 256u, (uint32_t)std::max(ctx->n_cu, 1) * 8u);
            IDIST_LAUNCH(range_allowed_init_kernel, grid_i, 256, 0, stream, st, ctx->al_size, ctx->al_start,
                         s_setof, ctx->al_first);
            HIPCHK(hipGetLastError());
            return IDIST_OK;
        };
        CHK(ladder_timed(ctx, 3, count_pass));
        np = 0;
        if (lad.n_rungs) { CHK(gather(0, d_last)); }
    }
    for (uint32_t r = 0; r < lad.n_rungs && np; r++) {
        const uint32_t ef = lad.E[r];
        bool ended = false;
        CHK(ladder_rung(idx, ctx, d_pq, np, ef, r, counters, &ended));
        if (ended) break;
        const uint32_t np_step = np;
        auto select_pass = [&]() -> idist_status {
            if (sets)
                IDIST_LAUNCH(range_allowed_select_kernel, std::min(np_step, 65536u), 64, 0, stream, st, s_bits, n, s_words, s_setof,
                             ctx->d_pid, reinterpret_cast<const uint32_t*>(ctx->d_dist.p), ctx->d_cnt, counters ? ctx->d_ctr.p : nullptr, ef,
                             d_list, np_step, r, step_cnt);
            else
                IDIST_LAUNCH(range_select_kernel, std::min(np_step, 65536u), 64, 0, stream, st, reinterpret_cast<const uint32_t*>(ctx->d_dist.p),
                             ctx->d_cnt, counters ? ctx->d_ctr.p : nullptr, ef, d_list, np_step, r, step_cnt);
            HIPCHK(hipGetLastError());
            return range_prefix(ctx, step_cnt, np_step, total, step_off);
        };
        CHK(ladder_timed(ctx, 3, select_pass));
        // the pending queries of the next rung, gathered BEFORE the copy so that one synchronisation reads the new total and their
        // number: the copy still needs this rung's list, so the lists alternate between two buffers (the rows of this rung stay
        // where they are until the copy has run; the next rows go to al_pq)
        uint32_t* next_list = d_list == ctx->al_list ? ctx->rg_list : ctx->al_list;
        CHK(ladder_pending(ctx, st.pending, nq, d_qk, kdim, next_list, 3, nullptr, r + 1u, d_last));
        uint64_t new_total = 0;
        HIPCHK(hipMemcpyAsync(&new_total, step_off + np_step, 8, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(&np, ctx->al_npend.p, 4, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (new_total > max_total) {
            char after[32];
            snprintf(after, sizeof(after), "rung %u", r);
            return range_too_many(new_total, max_total, after);
        }
        CHK(range_grow_keys(ctx, total, new_total));
        auto copy_pass = [&]() -> idist_status {
            if (sets)
                IDIST_LAUNCH(range_allowed_copy_kernel, std::min(np_step, 65536u), 64, 0, stream, st, s_bits, n, s_words, s_setof,
                             ctx->d_pid, reinterpret_cast<const uint32_t*>(ctx->d_dist.p), ef, d_list, np_step, step_cnt, step_off,
                             ctx->rg_keys);
            else
                IDIST_LAUNCH(range_copy_kernel, std::min(np_step, 65536u), 64, 0, stream, st, ctx->d_pid, reinterpret_cast<const uint32_t*>(ctx->d_dist.p),
                             ef, d_list, np_step, step_cnt, step_off, ctx->rg_keys);
            HIPCHK(hipGetLastError());
            return IDIST_OK;
        };
        CHK(ladder_timed(ctx, 3, copy_pass));                  // (enqueued, not waited for: the next launch follows it in stream order)
        total = new_total;
        d_list = next_list;
        d_pq = ctx->al_pq;
    }
    if (sets) { CHK(gather(kRungExact, nullptr)); }               // whoever is still pending: past its last rung, or the ladder ended
    if (np) {
        // step 3, exact: [0, n) cut into S segments, one wave per (pending query, segment); restricted: the 64-id windows of [0, n),
        // never narrower than one window
        const uint32_t S = exact_segments(ctx, np, n, ctx->knobs.range_segments);
        const uint64_t items = (uint64_t)np * S;
        CHK(ctx->d_cnt.grow((size_t)items * 4));
        CHK(ctx->rg_stepoff.grow((size_t)(items + 1) * 8));
        CHK(ctx->rg_exoff.grow((size_t)np * 8));
        CHK(ctx->rg_exlen.grow((size_t)np * 4));
        uint32_t* seg_cnt = ctx->d_cnt;
        uint64_t* seg_off = ctx->rg_stepoff;
        const size_t smem = smem_bytes(idx->L.stride, 0, false);
        if (smem > 64 * 1024) return fail(IDIST_ERR_INVALID_ARG, "dim needs %zu B of LDS per wave (> 64 KiB)", smem);
        const uint32_t grid = (uint32_t)std::min<uint64_t>(items, waves_cap);
        IndexView view = idx->view();
        auto scan_pass = [&](uint64_t* keys) -> idist_status {
            const uint32_t* d_lim = st.lim;
#define LAUNCH_AS(NB_, RS_, TAIL_)                                                                               \
    {                                                                                                            \
        auto kR = range_scan_kernel<NB_, RS_, TAIL_>;                                                            \
        IDIST_LAUNCH(kR, grid, 64, smem, stream, view, d_pq, np, d_list, d_lim, S, seg_cnt, seg_off, keys);      \
    }
#define LAUNCH_AS_SETS(NB_, RS_, TAIL_)                                                                          \
    {                                                                                                            \
        auto kA = range_allowed_scan_kernel<NB_, RS_, TAIL_>;                                                    \
        IDIST_LAUNCH(kA, grid, 64, smem, stream, view, d_pq, np, s_bits, n, s_words, d_list, s_setof, d_lim, S, seg_cnt, \
                     seg_off, keys);                                                                             \
    }
            if (sets) IDIST_DISPATCH(idx->L, LAUNCH_AS_SETS);
            else IDIST_DISPATCH(idx->L, LAUNCH_AS);
#undef LAUNCH_AS_SETS
#undef LAUNCH_AS
            HIPCHK(hipGetLastError());
            return IDIST_OK;
        };
        auto count_pass = [&]() -> idist_status {
            CHK(scan_pass(nullptr));
            CHK(range_prefix(ctx, seg_cnt, items, total, seg_off));
            IDIST_LAUNCH(range_close_kernel, std::min<uint32_t>((np + 255u) / 256u, 1024u), 256, 0, stream, st, d_list, np, S, seg_off,
                         ctx->rg_exoff, ctx->rg_exlen);
            HIPCHK(hipGetLastError());
            return IDIST_OK;
        };
        CHK(ladder_timed(ctx, 4, count_pass));
        uint64_t new_total = 0;
        std::vector<uint32_t> ex_len(np);
        HIPCHK(hipMemcpyAsync(&new_total, seg_off + items, 8, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(ex_len.data(), ctx->rg_exlen.p, (size_t)np * 4, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (new_total > max_total) return range_too_many(new_total, max_total, "the exact step");
        CHK(range_grow_keys(ctx, total, new_total));
        auto write_pass = [&]() -> idist_status { return scan_pass(ctx->rg_keys); };
        CHK(ladder_timed(ctx, 4, write_pass));
        const uint64_t max_len = *std::max_element(ex_len.begin(), ex_len.end());
        auto sort_pass = [&]() -> idist_status { return range_sort(ctx, np, max_len); };
        CHK(ladder_timed(ctx, 5, sort_pass));
        total = new_total;
    }
    *total_out = total;
    return IDIST_OK;
}

}  // namespace
}  // extern "C++"

idist_status idist_search_ctx_range_fetch(idist_search_ctx* ctx, uint32_t* out_pid, float* out_dist) {
    if (!ctx) return fail(IDIST_ERR_INVALID_ARG, "ctx is null");
    if (!ctx->rg_valid) return fail(IDIST_ERR_INVALID_ARG, "no range search results are held: call idist_search_batch_range first (a fetch hands them out once)");
    const uint64_t total = ctx->rg_total;
    if (total == 0) {
        ctx->rg_valid = false;
        return IDIST_OK;
    }
    if (!out_pid || !out_dist) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    CHK(ctx->rg_opid.grow(doubled_from(4096, (size_t)total * 4)));
    CHK(ctx->rg_odist.grow(doubled_from(4096, (size_t)total * 4)));
    RangeState st{};
    st.term = ctx->rg_term; st.count = ctx->rg_cnt; st.off = ctx->rg_off; st.nq = ctx->rg_nq;
    const uint32_t grid = std::min<uint32_t>(ctx->rg_nq, (uint32_t)std::max(ctx->n_cu, 1) * 64u);
    IDIST_LAUNCH(range_gather_kernel, grid, 64, 0, stream, st, ctx->rg_keys, ctx->rg_lims, (uint32_t)ctx->rg_metric,
                 ctx->rg_opid, ctx->rg_odist);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_pid, ctx->rg_opid.p, (size_t)total * 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(out_dist, ctx->rg_odist.p, (size_t)total * 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    ctx->rg_valid = false;
    return IDIST_OK;
}

idist_status idist_search_ctx_range_kernel_ms(idist_search_ctx* ctx, float* select_ms, float* scan_ms, float* sort_ms) {
    if (!ctx || !select_ms || !scan_ms || !sort_ms) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    *select_ms = ctx->al_ms[3];
    *scan_ms = ctx->al_ms[4];
    *sort_ms = ctx->al_ms[5];
    return IDIST_OK;
}

// ---- range search over a partitioned index: the parts' lists of any length merged on the device ----
extern "C++" {
namespace {

// c [nq] = the lists' counts summed (out_ctr [nq][3] or nullptr: their counters), lims [nq + 1] = its prefix sum; chunks: ceil(nq / 64)
// u64 of scratch.  Enqueued on `stream`.
idist_status launch_range_merge_counts(const RangeLists& L, uint32_t* c, uint32_t* out_ctr, uint64_t* chunks, uint64_t* lims, int n_cu,
                                       hipStream_t stream) {
    const uint32_t grid = std::min<uint32_t>((L.nq + 255u) / 256u, (uint32_t)std::max(n_cu, 1) * 8u);
    IDIST_LAUNCH(range_merge_counts_kernel, grid, 256, 0, stream, L, c, out_ctr);
    HIPCHK(hipGetLastError());
    return range_prefix_on(stream, chunks, c, L.nq, 0, lims);
}

// total = lims[nq] > 0 elements, a bounded tile of them per wave however they spread over queries and lists.  Enqueued on `stream`.
idist_status launch_range_merge(const RangeLists& L, const uint64_t* lims, uint64_t total, int32_t metric, const float* d_sq, float S,
                                uint32_t* out_pid, float* out_dist, int n_cu, hipStream_t stream) {
    uint32_t tile = kRangeMergeTile;
    if (const char* e = test_env("IDIST_RANGE_MERGE_TILE")) {      // test knob: the result must not depend on it
        const uint32_t t = (uint32_t)std::max(0, atoi(e));
        if (t >= 64u && t <= 65536u && t % 64u == 0u) tile = t;
    }
    const uint64_t tiles = (total + tile - 1u) / tile;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(tiles, (uint64_t)std::max(n_cu, 1) * 32u);   // the kernel strides over the rest
    IDIST_LAUNCH(range_merge_kernel, grid, 64, 0, stream, L, lims, total, tile, (uint32_t)metric, d_sq, S, out_pid, out_dist);
    HIPCHK(hipGetLastError());
    return IDIST_OK;
}

}  // namespace
}  // extern "C++"

idist_status idist_range_merge_device(const void* const* d_keys, const void* const* d_off, const void* const* d_cnt, uint32_t n_lists,
                                      uint32_t nq, const uint32_t* base, int32_t metric, const void* d_sq, float dot_bound,
                                      uint64_t capacity, void* d_lims, void* d_out_pid, void* d_out_dist, uint64_t* out_total,
                                      int32_t device, void* hip_stream) {
    if (n_lists == 0 || n_lists > kMergeMaxLists) return fail(IDIST_ERR_INVALID_ARG, "n_lists %u out of [1,%u]", n_lists, kMergeMaxLists);
    if (metric != IDIST_METRIC_L2SQ && metric != IDIST_METRIC_L2 && metric != IDIST_METRIC_COSINE && metric != IDIST_METRIC_DOT)
        return fail(IDIST_ERR_INVALID_ARG, "unknown metric %d", metric);
    if (!d_keys || !d_off || !d_cnt || !base || !d_lims || !out_total) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    if (nq && metric == IDIST_METRIC_DOT && !d_sq) return fail(IDIST_ERR_INVALID_ARG, "the inner-product metric reports with s(q): d_sq is null");
    for (uint32_t l = 0; nq && l < n_lists; l++)
        if (!d_off[l] || !d_cnt[l]) return fail(IDIST_ERR_INVALID_ARG, "list %u: null device pointer", l);
    *out_total = 0;
    CHK(check_device(device));
    HIPCHK(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)hip_stream;
    if (nq == 0) {
        HIPCHK(hipMemsetAsync(d_lims, 0, 8, stream));
        return IDIST_OK;
    }
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    RangeLists L{};
    L.n_lists = n_lists; L.nq = nq;
    for (uint32_t l = 0; l < n_lists; l++) {
        L.keys[l] = (const uint64_t*)d_keys[l]; L.off[l] = (const uint64_t*)d_off[l]; L.cnt[l] = (const uint32_t*)d_cnt[l];
        L.base[l] = base[l];
    }
    Scratch mem;
    uint32_t* c = nullptr;
    uint64_t* chunks = nullptr;
    CHK(mem.alloc(&c, nq));
    CHK(mem.alloc(&chunks, ((size_t)nq + 63u) / 64u));
    CHK(launch_range_merge_counts(L, c, nullptr, chunks, (uint64_t*)d_lims, launch_cus(prop.multiProcessorCount), stream));
    uint64_t total = 0;                                          // the one read-back: it checks the capacity
    HIPCHK(hipMemcpyAsync(&total, (const uint64_t*)d_lims + nq, 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    *out_total = total;
    if (total > capacity)
        return fail(IDIST_ERR_INVALID_ARG, "range merge: the lists hold %llu results, the output arrays %llu (nothing is written to them)",
                    (unsigned long long)total, (unsigned long long)capacity);
    if (total == 0) return IDIST_OK;
    if (!d_out_pid || !d_out_dist) return fail(IDIST_ERR_INVALID_ARG, "null device pointer");
    return launch_range_merge(L, (const uint64_t*)d_lims, total, metric, (const float*)d_sq, dot_bound, (uint32_t*)d_out_pid,
                              (float*)d_out_dist, launch_cus(prop.multiProcessorCount), stream);
}

// The range search over the parts behind its argument checks (p->rg_valid is false already).  src == nullptr: the plain call, which
// launches exactly what it always launched.  src: the restricted one — the sets staged per part as the restricted top-k call stages
// them (partitioned_stage_sets), every part's range_search_device given its own slice of them.
static idist_status partitioned_range_call(idist_partitioned* p, uint32_t ef, const float* queries, uint32_t nq, const float* radius,
                                           uint32_t n_radius, const SetsSource* src, int32_t max_rungs, uint64_t max_total, uint64_t* out_lims,
                                           uint32_t* out_rung, uint32_t* out_counters) {
    const size_t P = p->parts.size();
    const uint32_t N = p->base[P];
    if (out_rung) std::fill(out_rung, out_rung + (size_t)nq * P, (uint32_t)IDIST_RUNG_NONE);   // (empty parts keep it)
    if (nq == 0 || N == 0 || ef == 0) {                                      // nothing to find
        std::fill(out_lims, out_lims + nq + 1, (uint64_t)0);
        if (out_counters) memset(out_counters, 0, (size_t)nq * 12);
        p->rg_merge_ms = 0.0f;
        p->rg_valid = true;
        return IDIST_OK;
    }
    const bool counters = out_counters != nullptr;
    HIPCHK(hipSetDevice(p->merge_device));
    CHK(partitioned_prepare_report(p, queries, nq));
    // 1. the queries (DOT: and their s(q), the term of the parts' limits), once per distinct device that has something to search
    CHK(partitioned_upload_queries(p, queries, nq, true));
    if (src) {                                                   // ... and the restricted call's sets, every part's slice on its device
        p->al_slice_ms = 0.0f;
        CHK(partitioned_stage_sets(p, nq, *src));
    }
    // 2. the parts' searches block on the host once per rung: one thread per non-empty part, each with the part's own context and
    //    stream (step 3 of idist_partitioned_search_batch_allowed_sets).  Every part gets the caller's bound: its own total can never
    //    legitimately exceed the merged one.  A part on the merge device leaves its keys, offsets and counts where its context holds
    //    them; a part elsewhere sends them to the merge device by peer copies on its stream.
    std::vector<uint32_t> rungs(out_rung ? P * (size_t)nq : 0);
    CHK(partitioned_fan_out(p, [&](size_t i) -> idist_status {
        idist_partitioned::Part& pt = p->parts[i];
        idist_search_ctx* ctx = pt.ctx;
        const idist_partitioned::Dev& dv = p->devs[pt.dev_slot];
        const int32_t dev = dv.device;
        HIPCHK(hipSetDevice(dev));
        range_begin(pt.idx, ctx, nq);
        uint64_t total = 0;
        const RangeSets sets{ctx->al_bits, dv.d_setof, src ? src->n_sets : 0u, (pt.idx->n + 31u) / 32u};
        CHK(range_search_device(pt.idx, ctx, dv.d_q, dv.d_sq, nq, radius, n_radius, max_rungs, max_total, counters, &total, src ? &sets : nullptr));
        if (out_rung) HIPCHK(hipMemcpyAsync(rungs.data() + i * nq, ctx->al_orung.p, (size_t)nq * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (dev != p->merge_device) {
            HIPCHK(hipSetDevice(p->merge_device));               // (staging on the merge device only grows)
            CHK(pt.m_keys.grow(doubled_from(4096, (size_t)total * 8)));
            CHK(pt.m_off.grow((size_t)nq * 8));
            CHK(pt.m_cnt.grow((size_t)nq * 4));
            if (counters) CHK(pt.m_ctr.grow((size_t)nq * 12));
            HIPCHK(hipSetDevice(dev));
            if (total) HIPCHK(hipMemcpyPeerAsync(pt.m_keys, p->merge_device, ctx->rg_keys.p, dev, (size_t)total * 8, ctx->stream));
            HIPCHK(hipMemcpyPeerAsync(pt.m_off, p->merge_device, ctx->rg_off.p, dev, (size_t)nq * 8, ctx->stream));
            HIPCHK(hipMemcpyPeerAsync(pt.m_cnt, p->merge_device, ctx->rg_cnt.p, dev, (size_t)nq * 4, ctx->stream));
            if (counters) HIPCHK(hipMemcpyPeerAsync(pt.m_ctr, p->merge_device, ctx->al_octr.p, dev, (size_t)nq * 12, ctx->stream));
        }
        HIPCHK(hipStreamSynchronize(ctx->stream));
        CHK(attr_time_resolve(ctx));
        return ladder_times_resolve(ctx);
    }));
    if (src) partitioned_attr_times(p, *src);
    // 3. the union, on the merge device: the counts and lims, ONE read-back of the total (it checks max_total and sizes the output),
    //    the merge kernel straight into the flat arrays the fetch hands out
    HIPCHK(hipSetDevice(p->merge_device));
    RangeLists L{};
    L.nq = nq;
    for (size_t i = 0; i < P; i++) {
        const idist_partitioned::Part& pt = p->parts[i];
        if (!pt.ctx) continue;                               // an empty part hands in no list
        const bool here = p->devs[pt.dev_slot].device == p->merge_device;
        const uint32_t l = L.n_lists++;
        L.keys[l] = here ? pt.ctx->rg_keys.p : pt.m_keys.p;
        L.off[l] = here ? pt.ctx->rg_off.p : pt.m_off.p;
        L.cnt[l] = here ? pt.ctx->rg_cnt.p : pt.m_cnt.p;
        L.ctr[l] = !counters ? nullptr : (here ? pt.ctx->al_octr.p : pt.m_ctr.p);
        L.base[l] = p->base[i];
    }
    const int n_cu = p->parts[0].idx->n_cu;
    CHK(p->rm_c.grow((size_t)nq * 4));
    CHK(p->rm_lims.grow(((size_t)nq + 1) * 8));
    CHK(p->rm_chunks.grow(doubled_from(256, (((size_t)nq + 63u) / 64u) * 8)));
    if (counters) CHK(p->o_ctr.grow((size_t)nq * 12));
    HIPCHK(hipEventRecord(p->ev0, p->stream));
    CHK(launch_range_merge_counts(L, p->rm_c, counters ? p->o_ctr.p : nullptr, p->rm_chunks, p->rm_lims, n_cu, p->stream));
    HIPCHK(hipEventRecord(p->ev1, p->stream));
    uint64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, p->rm_lims + nq, 8, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    float ms_counts = 0.0f, ms_merge = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms_counts, p->ev0, p->ev1));
    if (total > max_total) return range_too_many(total, max_total, "the merge");
    if (total) {
        CHK(p->rm_opid.grow(doubled_from(4096, (size_t)total * 4)));
        CHK(p->rm_odist.grow(doubled_from(4096, (size_t)total * 4)));
        HIPCHK(hipEventRecord(p->ev0, p->stream));
        CHK(launch_range_merge(L, p->rm_lims, total, p->metric, p->d_sq, p->dot_S, p->rm_opid, p->rm_odist, n_cu, p->stream));
        HIPCHK(hipEventRecord(p->ev1, p->stream));
    }
    HIPCHK(hipMemcpyAsync(out_lims, p->rm_lims, ((size_t)nq + 1) * 8, hipMemcpyDeviceToHost, p->stream));
    if (counters) HIPCHK(hipMemcpyAsync(out_counters, p->o_ctr, (size_t)nq * 12, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    if (total) HIPCHK(hipEventElapsedTime(&ms_merge, p->ev0, p->ev1));
    p->rg_merge_ms = ms_counts + ms_merge;
    partitioned_transpose_rungs(p, rungs, nq, out_rung);
    p->rg_total = total;
    p->rg_valid = true;
    return IDIST_OK;
}

idist_status idist_partitioned_search_batch_range(idist_partitioned* p, const float* queries, uint32_t nq, const float* radius,
                                                  uint32_t n_radius, int32_t max_rungs, uint64_t max_total, uint64_t* out_lims,
                                                  uint32_t* out_rung, uint32_t* out_counters) {
    if (!p) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    p->rg_valid = false;                                                     // whatever happens next, the previous results are gone
    p->rg_total = 0;
    uint32_t ef = 0;
    CHK(partitioned_check(p, &ef));
    CHK(check_range_args(queries, nq, radius, n_radius, max_rungs, out_lims));
    return partitioned_range_call(p, ef, queries, nq, radius, n_radius, nullptr, max_rungs, max_total, out_lims, out_rung, out_counters);
}

// ---- restricted range search over the parts: the missing cell ----
idist_status idist_partitioned_search_batch_range_allowed_sets(idist_partitioned* p, const float* queries, uint32_t nq, const float* radius,
                                                               uint32_t n_radius, const uint32_t* allow_bits, uint32_t n_sets,
                                                               const uint32_t* set_of, int32_t max_rungs, uint64_t max_total,
                                                               uint64_t* out_lims, uint32_t* out_rung, uint32_t* out_counters) {
    if (!p) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    p->rg_valid = false;                                                     // whatever happens next, the previous results are gone
    p->rg_total = 0;
    uint32_t ef = 0;
    CHK(partitioned_check(p, &ef));
    CHK(check_range_args(queries, nq, radius, n_radius, max_rungs, out_lims));
    CHK(check_sets_args(n_sets, set_of, nq));
    if (nq && p->base[p->parts.size()] && !allow_bits) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    std::vector<uint32_t> identity;
    SetsSource src;
    src.bits = allow_bits; src.n_sets = n_sets; src.set_of = set_of_or_identity(set_of, nq, &identity);
    return partitioned_range_call(p, ef, queries, nq, radius, n_radius, &src, max_rungs, max_total, out_lims, out_rung, out_counters);
}

idist_status idist_partitioned_search_batch_range_attr(idist_partitioned* p, const idist_attr* attr, const float* queries, uint32_t nq,
                                                       const float* radius, uint32_t n_radius, const uint32_t* lo, const uint32_t* hi,
                                                       uint32_t n_cond, int32_t max_rungs, uint64_t max_total, uint64_t* out_lims,
                                                       uint32_t* out_rung, uint32_t* out_counters) {
    if (!p) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    p->rg_valid = false;                                                     // whatever happens next, the previous results are gone
    p->rg_total = 0;
    uint32_t ef = 0;
    CHK(partitioned_check(p, &ef));
    CHK(check_partitioned_attr(p, attr));
    CHK(check_range_args(queries, nq, radius, n_radius, max_rungs, out_lims));
    CHK(check_cond_args(lo, hi, n_cond, nq));
    AttrConds g;
    attr_group(lo, hi, nq ? n_cond : 0u, nq, &g);
    const SetsSource src = g.source(attr);
    return partitioned_range_call(p, ef, queries, nq, radius, n_radius, &src, max_rungs, max_total, out_lims, out_rung, out_counters);
}

idist_status idist_partitioned_search_batch_range_match(idist_partitioned* p, const idist_attr* attr, const float* queries, uint32_t nq,
                                                        const float* radius, uint32_t n_radius, const idist_attr_conds* conds,
                                                        int32_t max_rungs, uint64_t max_total, uint64_t* out_lims, uint32_t* out_rung,
                                                        uint32_t* out_counters) {
    if (!p) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    p->rg_valid = false;                                                     // whatever happens next, the previous results are gone
    p->rg_total = 0;
    uint32_t ef = 0;
    CHK(partitioned_check(p, &ef));
    CHK(check_partitioned_attr(p, attr));
    CHK(check_range_args(queries, nq, radius, n_radius, max_rungs, out_lims));
    CHK(check_match_args(conds, nq, attr->n_cols));
    MatchConds g;
    match_group(conds, nq ? conds->n_cond : 0u, nq, &g);
    const SetsSource src = g.source(attr);
    return partitioned_range_call(p, ef, queries, nq, radius, n_radius, &src, max_rungs, max_total, out_lims, out_rung, out_counters);
}

idist_status idist_partitioned_range_fetch(idist_partitioned* p, uint32_t* out_pid, float* out_dist) {
    if (!p) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    if (!p->rg_valid)
        return fail(IDIST_ERR_INVALID_ARG, "no range search results are held: call idist_partitioned_search_batch_range first (a fetch hands them out once)");
    const uint64_t total = p->rg_total;
    if (total == 0) {
        p->rg_valid = false;
        return IDIST_OK;
    }
    if (!out_pid || !out_dist) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    HIPCHK(hipSetDevice(p->merge_device));
    HIPCHK(hipMemcpyAsync(out_pid, p->rm_opid, (size_t)total * 4, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipMemcpyAsync(out_dist, p->rm_odist, (size_t)total * 4, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    p->rg_valid = false;
    return IDIST_OK;
}

idist_status idist_partitioned_last_range_merge_ms(idist_partitioned* p, float* ms) {
    if (!p || !ms) return fail(IDIST_ERR_INVALID_ARG, "null argument");
    if (p->rg_merge_ms < 0.0f) return fail(IDIST_ERR_INVALID_ARG, "no range search has run through this object yet");
    *ms = p->rg_merge_ms;
    return IDIST_OK;
}

idist_status idist_normalize_batch(const float* rows, uint32_t n, uint32_t dim, float* out_rows, float* out_norm2, int32_t device) {
    if (dim == 0 || dim > 65536) return fail(IDIST_ERR_INVALID_ARG, "dim %u out of [1,65536]", dim);
    if (n == 0) return IDIST_OK;
    if (!rows || !out_rows) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    CHK(check_device(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    Scratch mem;
    float *d_x = nullptr, *d_s = nullptr;
    const size_t xb = (size_t)n * dim * 4;
    CHK(mem.alloc(&d_x, xb / 4));
    if (out_norm2) CHK(mem.alloc(&d_s, n));
    HIPCHK(hipMemcpy(d_x, rows, xb, hipMemcpyHostToDevice));
    CHK(launch_normalize(d_x, d_x, n, dim, dim, 0u, d_s, launch_cus(prop.multiProcessorCount), nullptr));
    HIPCHK(hipMemcpy(out_rows, d_x, xb, hipMemcpyDeviceToHost));
    if (out_norm2) HIPCHK(hipMemcpy(out_norm2, d_s, (size_t)n * 4, hipMemcpyDeviceToHost));
    return IDIST_OK;
}

idist_status idist_dot_augment_batch(const float* rows, uint32_t n, uint32_t dim, float bound_in, float* out_rows, float* out_norm2,
                                     float* out_bound, int32_t device) {
    if (dim == 0 || dim > 65535) return fail(IDIST_ERR_INVALID_ARG, "dim %u out of [1,65535]", dim);
    if (!(bound_in >= 0.0f && bound_in < INFINITY)) return fail(IDIST_ERR_INVALID_ARG, "dot_bound %g is not a finite number >= 0", (double)bound_in);
    if (n && !rows) return fail(IDIST_ERR_INVALID_ARG, "null pointer");
    CHK(check_device(device));
    if (n == 0) { if (out_bound) *out_bound = bound_in; return IDIST_OK; }
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    const uint32_t kdim = dim + 1u;
    Scratch mem;
    float *d_x = nullptr, *d_s = nullptr, *d_a = nullptr;
    const size_t xb = (size_t)n * dim * 4, ab = (size_t)n * kdim * 4;
    CHK(mem.alloc(&d_x, xb / 4));
    CHK(mem.alloc(&d_s, n));
    if (out_rows) CHK(mem.alloc(&d_a, ab / 4));
    HIPCHK(hipMemcpy(d_x, rows, xb, hipMemcpyHostToDevice));
    float S = bound_in;
    CHK(dot_augment_device(d_x, d_a, n, dim, kdim, 0u, &S, d_s, launch_cus(prop.multiProcessorCount)));   // (natural x~ rows: stride kdim, no blocks)
    if (out_rows) HIPCHK(hipMemcpy(out_rows, d_a, ab, hipMemcpyDeviceToHost));
    if (out_norm2) HIPCHK(hipMemcpy(out_norm2, d_s, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (out_bound) *out_bound = S;
    return IDIST_OK;
}

}  // extern "C"
