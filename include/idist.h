/*
 * idist.h — C ABI of libidist.so, the MI355X (gfx950) HNSW build+search engine
 * that sits under instant-distance's Builder / Hnsw / HnswMap / Search / Point
 * API (the drop-in boundary).
 *
 * The reference has NO FFI of its own: its boundary is the public Rust API.
 * Each entry point below names the reference item it stands in for
 * (paths relative to /root/reference/, core/ = instant-distance/src/).  The
 * Rust-side binding a maintainer adds is shown in INTEGRATION.md and shipped as
 * source in instant-distance_amd/rust-shim/.
 *
 * Conventions
 *   - plain pointers and sizes only; the caller owns every host buffer, the
 *     library owns all device memory behind the opaque handles;
 *   - every call returns an idist_status (0 = ok); idist_last_error() gives a
 *     thread-local message.  The reference API is infallible (it only panics at
 *     core/lib.rs:256 and :148) so the shim `expect()`s these;
 *   - points are handed over ALREADY IN PointId ORDER: the seed -> permutation
 *     step (core/lib.rs:214,257-270, `rand` crate) stays on the caller's side;
 *   - an idist_index is immutable after build/import and may be shared by any
 *     number of threads; every idist_search_ctx owns its own stream + scratch
 *     (the role of `&mut Search`, core/lib.rs:352-356).
 *   - there is no CPU fallback: without a gfx950 device every compute entry
 *     point fails with IDIST_ERR_NO_DEVICE.
 *
 * Environment: libidist.so reads exactly three variables, all host-side behaviour, sampled once per context —
 *   IDIST_COMBINE=0         every scalar host-pointer call makes its own launch (no riding along in another thread's launch)
 *   IDIST_SYNC=stream       narrow host-pointer calls wait with hipStreamSynchronize instead of for the kernel's completion word
 *   IDIST_KERNEL_EVENTS=0   no HIP events around the search kernels (idist_search_ctx_kernel_times then has nothing)
 * — and nothing in the environment can change which kernels it runs or which graph it builds.  The knobs that select other
 * implementations of the same decisions (IDIST_WALK, IDIST_VISITED, IDIST_TAB_*, IDIST_BUILD_*, ...) exist for the parity tests
 * and A/B measurements and are compiled into the TEST build of the same sources only (libidist_variants.so, `make variants`;
 * DESIGN.md's appendix lists them).  The library never edits the environment either: GPU_MAX_HW_QUEUES (one hardware queue per
 * searching thread's stream) is the host's to set before its first HIP call.
 */
#ifndef IDIST_H
#define IDIST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IDIST_M 32u                 /* core/lib.rs:787 */
#define IDIST_M2 64u                /* ZeroNode slots, core/types.rs:83-85 */
#define IDIST_INVALID 0xFFFFFFFFu   /* PointId INVALID, core/types.rs:293 */
#define IDIST_MAX_LAYERS 64u
#define IDIST_MAX_EF 4096u

typedef int32_t idist_status;
enum {
    IDIST_OK = 0,
    IDIST_ERR_INVALID_ARG = 1,
    IDIST_ERR_NO_DEVICE = 2,      /* no gfx950 GPU visible: there is no CPU path */
    IDIST_ERR_HIP = 3,            /* HIP runtime error, see idist_last_error() */
    IDIST_ERR_UNSUPPORTED = 4,    /* option the GPU engine does not implement (yet) */
    IDIST_ERR_BAD_GRAPH = 5,      /* imported adjacency violates the reference's invariants */
    IDIST_ERR_TIE_OVERFLOW = 6,   /* device-pointer launches only: the tie region overflowed, enqueue the batch again (idist_config.tie_policy) */
    IDIST_ERR_INTERNAL = 7        /* device-side guard tripped */
};

enum { IDIST_TIES_STRICT = 0, IDIST_TIES_DROP = 1 };

enum {
    IDIST_METRIC_L2SQ = 0, /* FloatArray::distance, instant-distance-py/src/lib.rs:378-421 */
    IDIST_METRIC_L2 = 1,   /* sqrt of it: tests/all.rs:93-97, examples/colors.rs:21-25 */
    IDIST_METRIC_COSINE = 2, /* cosine distance 1 - cos (no counterpart in the reference), DEFINED through L2SQ: with s(x) = the canonical
                              L2SQ distance of x to the origin, r = sqrtf(s) and x^ = x / r coordinate by coordinate (f32, correctly
                              rounded; x^ = x when r is not a positive finite number: zero rows, NaN / inf, s overflowed or underflowed),
                              an index with this metric over rows X IS the L2SQ index over X^ — same graph, same ids, order, counts and
                              counters for a query q as the L2SQ search of q^ — and every distance it reports is 0.5f * d, one f32
                              multiply of the canonical L2SQ distance d (|q^ - x^|^2 / 2 = 1 - cos).  Rows are normalised where they become
                              the index's device copy (build, build_device, import), queries per call; the caller's buffers are never
                              written.  idist_index_device_buffers / idist_replicate* hand on rows that already are x^. */
    /* (3 is not assigned and is refused) */
    IDIST_METRIC_DOT = 4    /* inner product, nearest = LARGEST q.x (no counterpart in the reference), DEFINED through L2SQ over one more
                              coordinate.  dim is the caller's dimension everywhere in this ABI, kdim = dim + 1 what the index stores.
                              1. s(x) = the canonical L2SQ distance of x to the origin over its dim coordinates (what
                                 idist_normalize_batch returns as out_norm2; NOT taken over kdim coordinates).  A row is finite when
                                 s(x) is neither NaN nor inf.
                              2. S = idist_config.dot_bound if that is > 0, else the maximum of s(x) over the finite rows (0 when there
                                 is none).  A given bound must be finite and >= every finite s(x): IDIST_ERR_INVALID_ARG otherwise,
                                 naming a row.
                              3. e(x) = sqrtf(S - s(x)) for finite rows (one f32 subtraction, a correctly rounded square root), else 0.
                              4. x~ = (x, e(x)), q~ = (q, 0), both of length kdim: |q~ - x~|^2 = |q|^2 + S - 2 q.x.
                              5. An index with this metric over rows X IS the L2SQ index over X~ - same graph, same ids, order, counts
                                 and counters for a query q as the L2SQ search of q~.
                              6. With d the canonical L2SQ distance and t = s(q) + S (one f32 add), every reported distance is
                                 0.5f * (d - t) in IEEE f32, approximately -q.x; a d that is +inf (the padding) or NaN is reported
                                 unchanged.  It is non-decreasing in d (nearest first still holds, possibly with ties).  Its absolute
                                 error is of the order eps * (|q|^2 + S), NOT eps * |q.x|: one giant-norm outlier row coarsens every
                                 other distance.  idist_filter_bound_batch: the transformed bound is a lower bound of the reported
                                 value; "no bound" (raw 0) becomes the trivial bound -t / 2.
                              Rows are augmented where they become the index's device copy (build, build_device, import), queries per
                              call; the caller's buffers are never written.  idist_index_device_buffers / idist_replicate* hand on rows
                              that already are x~ (row_stride is that of kdim), and a replication target needs the same S:
                              idist_index_alloc takes it from idist_config.dot_bound (0 there is refused).  Every part of a partitioned
                              index must hold the same S bit for bit.  dim <= 65535. */
};

/* Builder fields, core/lib.rs:23-31 (defaults :101-128). */
typedef struct idist_config {
    uint32_t ef_search;         /* Builder::ef_search, default 100 */
    uint32_t ef_construction;   /* Builder::ef_construction, default 100 */
    float ml;                   /* Builder::ml, default 1/ln(32) */
    int32_t has_heuristic;      /* Builder::select_heuristic(Some/None), default Some */
    int32_t extend_candidates;  /* Heuristic::extend_candidates, default false.  true: core/lib.rs:648-664 without the
                                   locks that make it deadlock upstream (:649 vs :438) = the oracle's restatement;
                                   the build is then sequential whatever max_batch says (one insertion per launch) */
    int32_t keep_pruned;        /* Heuristic::keep_pruned, default true */
    int32_t metric;             /* IDIST_METRIC_* (the Point::distance the caller would supply) */
    uint32_t max_batch;         /* build scheduling: 1 = strictly sequential insertion (the
                                   deterministic contract = reference with one rayon thread);
                                   0 = library default; k = at most k concurrent inserts per
                                   step (the rayon for_each of core/lib.rs:316-318). */
    int32_t tie_policy;         /* IDIST_TIES_*: what happens when more un-expanded candidates sit exactly at the furthest
                                   distance of a full `nearest` than the engine's tie region holds (mass duplicates, dense
                                   integer grids).  The reference's candidate heap is unbounded (core/lib.rs:564).
                                   STRICT (default): the result is ALWAYS the reference's.  The region grows on demand — a
                                   build that overflows is repeated with 8x the region, a host-pointer search batch is
                                   searched again with 4x — and beyond 4096 entries the ties that do not fit go to a bag
                                   in HBM and come back in (distance, pid) order: unbounded like the reference's heap, slow
                                   only on data that needs it.  IDIST_ERR_TIE_OVERFLOW is returned in ONE place only:
                                   idist_search_ctx_status after a device-pointer launch (idist_search_batch_device cannot
                                   re-run a launch it did not wait for); that context uses the larger region / the bags
                                   from its next launch on, so the caller enqueues the same batch again.
                                   DROP: keep the configured region, never expand the ties that do not fit, go on —
                                   deterministic, flagged in idist_build_stats.tie_overflow /
                                   idist_search_ctx_tie_overflowed, no longer bit-identical on such data. */
    uint32_t tie_capacity;      /* initial size of that tie region, 0 = 64 (the default), at most 4096.  It lives in LDS
                                   next to `nearest` (8 B per entry): a larger one spares such data the repeated launch at
                                   the price of fewer resident waves per CU.  (HBM bags: n keys per query slot, as many
                                   slots as fit 1 GiB.) */
    float dot_bound;            /* IDIST_METRIC_DOT only (ignored otherwise): the bound S on the rows' squared norms, 0 (the default) =
                                   derive it from the rows.  idist_index_get_info reports the S in use. */
} idist_config;

typedef struct idist_index idist_index;
typedef struct idist_search_ctx idist_search_ctx;

typedef struct idist_index_info {
    uint32_t n, dim;
    uint32_t row_stride;        /* floats per stored row (blocked layout) */
    uint32_t n_upper;           /* Hnsw.layers.len() */
    uint32_t ef_search;
    int32_t metric;
    int32_t device;
    uint32_t layer_len[IDIST_MAX_LAYERS]; /* layer_len[l-1] = rows of layers[l-1], l = 1..n_upper */
    uint32_t tie_capacity;      /* the tie region the build ended up using (see idist_config.tie_capacity) */
    float dot_bound;            /* IDIST_METRIC_DOT: the bound S in use (given or derived); 0 for every other metric */
    int32_t filter_format;      /* the reject filter's compact rows a wide search of this index reads:
                                   IDIST_FILTER_FORMAT_NONE / _IDENTITY (one byte per stored float) / _PRINCIPAL (64-byte rows in a
                                   principal basis: thin search walks of low-rank data).  One deterministic choice per index. */
    uint64_t filter_bytes;           /* device memory of the identity table (0: this index runs unfiltered) ... */
    uint64_t filter_principal_bytes; /* ... and of the principal one, 64 B per row on top (0: not made, or dropped by the policy) */
    uint64_t filter_inline_bytes;    /* ... and of the principal rows stored once more with the adjacency, 4096 B per point: made at the first
                                        wide search of an index in the PRINCIPAL format (0: not made — another format, above the cap of
                                        8 GiB, or no memory; the walks then read the principal table itself) */
} idist_index_info;
enum { IDIST_FILTER_FORMAT_NONE = 0, IDIST_FILTER_FORMAT_IDENTITY = 1, IDIST_FILTER_FORMAT_PRINCIPAL = 2 };

/* Raw device views (for RCCL replication by the host: torch.distributed / ncclBroadcast). */
typedef struct idist_device_buffers {
    void* points;  size_t points_bytes;  /* f32 [n][row_stride], blocked layout */
    void* zero;    size_t zero_bytes;    /* u32 [n][64] */
    void* upper;   size_t upper_bytes;   /* u32 [sum layer_len][32], layer 1 first */
} idist_device_buffers;

/* Work counters that define the algorithmic bytes. */
typedef struct idist_build_stats {
    uint64_t n_dist;        /* descent distance evaluations (Search::push past `visited`) */
    uint64_t n_exp0;        /* zero-array expansions */
    uint64_t n_expU;        /* snapshot (UpperNode) expansions */
    uint64_t n_sel_pairs;   /* candidate pairs of select_heuristic DECIDED here (by the Gram-matrix filter, a memoised
                               verdict or the canonical distance) — this engine's work, not the reference's count */
    uint64_t n_heur_rows;   /* candidate rows staged for select_heuristic */
    uint64_t n_updates;     /* neighbour rows rewritten (ZeroNode::rewrite) */
    uint64_t n_updates_fast; /* ... of which through the memoised re-selection */
    uint64_t n_updates_full; /* ... of which through the full re-selection */
    uint64_t n_batches;
    double seconds;         /* device time of the whole build (HIP events) */
    uint64_t tie_overflow;  /* 1 if the tie capacity was exceeded during the build (only with IDIST_TIES_DROP) */
    uint64_t n_heur_ref;    /* distance calls of select_heuristic / add_neighbor_heuristic exactly as the reference makes them
                               (early-exit `any`, core/lib.rs:676-679; the pushes of :626-629) — available (non-zero) only when
                               the whole build ran through the reference-order kernels: max_batch = 1 with
                               IDIST_BUILD_A2=tile IDIST_BUILD_NO_FAST=1, or extend_candidates; tests compare it with the oracle */
    uint64_t n_filter_examined; /* descent pushes (of n_dist) the reject filter looked up in the compact copy of the rows first ... */
    uint64_t n_filter_rejected; /* ... and of those, the candidates whose f32 row was never fetched (0 / 0: unfiltered descents) */
    uint64_t filter_row_bytes;  /* bytes of one compact row (0: unfiltered descents): what an examined candidate costs instead of 4 * dim */
} idist_build_stats;

/* ---- library ------------------------------------------------------------ */
const char* idist_last_error(void);
const char* idist_version(void);
idist_status idist_device_count(int32_t* out);
/* Builder::default(), core/lib.rs:101-113 (seed stays with the caller). */
idist_status idist_default_config(idist_config* cfg);
/* Layer sizing of Hnsw::new, core/lib.rs:238-250 (f32 multiply + truncation).
 * cum[l] = nodes present on layer l, cum[0] = n; returns the layer count in *n_layers. */
idist_status idist_layer_sizes(uint32_t n, float ml, uint32_t* cum, uint32_t cap, uint32_t* n_layers);

/* Host helper (no GPU): the shuffle of Hnsw::new, core/lib.rs:214,257-270 — keys drawn with
 * SmallRng::seed_from_u64(seed).random_range(0..n), sort_unstable by (key, index).
 * out_pid[orig] = PointId, order[pid] = original index (either may be NULL).
 * PARITY UNPINNED: the `rand` crate is not part of /root/reference (Cargo.lock is git-ignored);
 * this restates xoshiro256++ / SplitMix64 seeding / widening-multiply range sampling.  A Rust
 * caller keeps using the real crate and passes points in PointId order. */
idist_status idist_permutation(uint64_t seed, uint32_t n, uint32_t* out_pid, uint32_t* order);

/* ---- index -------------------------------------------------------------- */
/* Builder::build_hnsw / Hnsw::new, core/lib.rs:83-85, 209-345 (after the permutation):
 * inserts points 1..n per layer range (Construction::insert, :437-528, select_heuristic
 * :636-698) on the GPU.  `points` is host memory, row-major n x dim, PointId order. */
idist_status idist_index_build(const float* points, uint32_t n, uint32_t dim,
                               const idist_config* cfg, int32_t device, idist_index** out);
/* Same, points already resident on `device` (row-major n x dim f32). */
idist_status idist_index_build_device(const void* d_points, uint32_t n, uint32_t dim,
                                      const idist_config* cfg, int32_t device, idist_index** out);
idist_status idist_index_build_stats(const idist_index* idx, idist_build_stats* out);

/* Builder::progress (core/lib.rs:70-75 behind the `indicatif` feature; the bar is advanced at :217-221,
 * :306-309, :332-334, :520-526).  No callbacks cross this ABI, so progress is a pollable object: create it,
 * arm it on the thread that is about to call idist_index_build*, and read it from any other thread while
 * that (blocking) call runs.  `total` = points.len() (bar.set_length, :219), `done` = points inserted so
 * far (the bar's position), `layer` = the layer being built (the bar's message, :307), -1 before the first
 * and after the last.  The device advances it after every build step. */
typedef struct idist_progress idist_progress;
idist_status idist_progress_new(idist_progress** out);
void idist_progress_free(idist_progress* p);
/* the next idist_index_build / idist_index_build_device call made by THIS thread reports into `p` */
idist_status idist_progress_watch_next_build(idist_progress* p);
idist_status idist_progress_get(const idist_progress* p, uint64_t* done, uint64_t* total, int32_t* layer);

/* Adopt an existing graph: the fields of `struct Hnsw`, core/lib.rs:194-199
 * (points, zero: Vec<ZeroNode>, layers: Vec<Vec<UpperNode>>).  Rows are validated
 * against the reference's invariants (ids < n, no duplicate before the first INVALID). */
idist_status idist_index_import(const float* points, uint32_t n, uint32_t dim,
                                const idist_config* cfg, const uint32_t* zero,
                                const uint32_t* const* layers, const uint32_t* layer_len,
                                uint32_t n_upper, int32_t device, idist_index** out);
/* Empty index with the layer structure `layer_len` (replication target). */
idist_status idist_index_alloc(uint32_t n, uint32_t dim, const idist_config* cfg,
                               const uint32_t* layer_len, uint32_t n_upper, int32_t device,
                               idist_index** out);
/* Copy the graph back to host: zero must hold n*64, layers[l-1] layer_len[l-1]*32 u32. */
idist_status idist_index_export(const idist_index* idx, uint32_t* zero, uint32_t* const* layers);
idist_status idist_index_get_info(const idist_index* idx, idist_index_info* out);
idist_status idist_index_device_buffers(const idist_index* idx, idist_device_buffers* out);
/* Hnsw.ef_search is a field of the index (core/lib.rs:195); bench sweeps change it. */
idist_status idist_index_set_ef_search(idist_index* idx, uint32_t ef_search);
void idist_index_free(idist_index* idx);

/* ---- search ------------------------------------------------------------- */
/* Search::default(), core/lib.rs:767-778: reusable scratch (visited set, W, candidates) for up to `slots`
 * queries in flight.  The visited set is one BIT per point and slot (core/types.rs:13-59 keeps a byte and a
 * generation; membership is all that is observable).  slots = 0: like the reference's Search, which sizes its
 * scratch on first use (core/lib.rs:363), the context starts with ONE slot (n/8 bytes) and grows to what the
 * batches it is given need, at most a full chip (16 waves per CU = 4096 slots: 512 MB at 1M points; the default walk
 * keeps the visited set of a query in LDS and touches this bitmap only when it overflows).
 * A context is bound to the index it was created for (by identity, not by address). */
idist_status idist_search_ctx_new(const idist_index* idx, uint32_t slots, idist_search_ctx** out);
void idist_search_ctx_free(idist_search_ctx* ctx);
/* Back `slots` query slots now (Vec::reserve on the Search's scratch).  Growing is the one operation of a context that
 * synchronises the whole device and allocates (the old bitmaps may still be in use by launches on any stream): a launch
 * wider than the slots a context has grows it first, so a caller of idist_search_batch_device who needs launches that
 * never synchronise (stream capture, other contexts busy on the device) reserves min(widest batch, a full chip) up front. */
idist_status idist_search_ctx_reserve(idist_search_ctx* ctx, uint32_t slots);

/* Hnsw::search, core/lib.rs:352-383, for nq queries at once (nq == 1 backs the scalar
 * call; scalar calls from many threads — one context each, the reference's `&mut Search` per thread — are combined into
 * few launches once more than eight are in flight on the index: same results, higher aggregate rate).  Results are Search.nearest: <= ef_search (pid, distance) pairs, nearest first
 * (the caller's `.take(k)` is a prefix).  out_pid/out_dist: nq*ef_search, padded with
 * IDIST_INVALID / +inf; out_count: nq; out_counters (optional): nq*3
 * {n_dist, n_exp0, n_expU} per query.  Host pointers; blocks until done. */
idist_status idist_search_batch(const idist_index* idx, idist_search_ctx* ctx,
                                const float* queries, uint32_t nq, uint32_t* out_pid,
                                float* out_dist, uint32_t* out_count, uint32_t* out_counters);
/* Same with every pointer in device memory, enqueued on `hip_stream` (a hipStream_t, may
 * be NULL) without synchronising: inputs/outputs stay resident in HBM.  A context is one
 * `&mut Search`: its launches must be ordered among themselves (one stream, or explicit
 * dependencies) — they share its visited slots and its work queue; use one context per
 * concurrent stream.  Batches of up to ~100 queries through idist_search_batch (host
 * pointers) cross PCIe through a pinned buffer owned by the context, without copy calls. */
idist_status idist_search_batch_device(const idist_index* idx, idist_search_ctx* ctx,
                                       const void* d_queries, uint32_t nq, void* d_out_pid,
                                       void* d_out_dist, void* d_out_count, void* d_out_counters,
                                       void* hip_stream);
/* Device-side status of the last launches on ctx (after the stream is synchronised). */
idist_status idist_search_ctx_status(idist_search_ctx* ctx);
/* IDIST_TIES_DROP only: *out = 1 if a search since the last call exceeded the tie capacity (then reset). */
idist_status idist_search_ctx_tie_overflowed(idist_search_ctx* ctx, int32_t* out);
/* Diagnostics of the walk's reject filter: wide batches on indexes the filter applies to look every new
 * candidate up in a one-byte-per-coordinate copy of the rows first and fetch the f32 row only of those that copy cannot prove to
 * lie beyond `nearest`'s furthest entry — the candidates `Search::push` turns down at core/lib.rs:712-714 without using their
 * distance.  Results and the counters of idist_search_batch are the reference's either way; these two numbers say how many
 * candidates the filter examined and how many f32 rows it spared, summed over the searches of this context since the last
 * reset (bench.py derives the bytes a launch really requests from them).  Synchronise the context's stream first. */
idist_status idist_search_ctx_filter_counts(idist_search_ctx* ctx, uint64_t* examined, uint64_t* rejected, int32_t reset);
/* ... and the part of both that the walks read from the 64-byte principal rows (idist_index_info.filter_format): a query whose energy
 * lies mostly outside the index's basis is served from the identity rows inside the same launch, so what a launch requested is
 * principal_examined * 64 + (examined - principal_examined) * identity row bytes + (pushes - rejected) * 4 * dim.  Own reset. */
idist_status idist_search_ctx_filter_principal_counts(idist_search_ctx* ctx, uint64_t* examined, uint64_t* rejected, int32_t reset);
/* ... and, for an index with idist_index_info.filter_inline_bytes: the 4096-byte blocks the walks requested (prefetches for a wrong
 * guess included) and the blocks they tested.  The candidates counted by filter_principal_counts were then read as part of these blocks:
 * a launch requested blocks_requested * 4096 bytes of compact rows for them instead of principal_examined * 64.  Own reset. */
idist_status idist_search_ctx_filter_inline_counts(idist_search_ctx* ctx, uint64_t* blocks_requested, uint64_t* blocks_used, int32_t reset);
/* HIP-event duration of the last search kernel launched through ctx, milliseconds. */
idist_status idist_search_ctx_last_kernel_ms(idist_search_ctx* ctx, float* ms);
/* Durations (ms) of the most recent search-kernel launches through ctx, oldest first, measured
 * with HIP events recorded on the launch stream around each kernel (a ring of IDIST_EVENT_RING
 * pairs; no synchronisation happens until this call).  *n_out = number written (<= cap). */
#define IDIST_EVENT_RING 64u
idist_status idist_search_ctx_kernel_times(idist_search_ctx* ctx, float* ms, uint32_t cap, uint32_t* n_out);

/* ---- several GPUs of one node --------------------------------------------------- */
/* `Hnsw` is Sync — Hnsw::search takes &self and every mutable bit lives in the caller's Search
 * (core/lib.rs:352-356) — so the reference shares ONE index between all its threads.  Across GPUs the index
 * is replicated once and the queries are block-partitioned; the build itself does not shard (every insert
 * reads and mutates one graph): it runs on one GPU and is replicated ("replicas only").
 *
 * idist_replicate: replicas[i] receives a copy of `root` on devices[i], device to device over xGMI
 * (hipMemcpyPeerAsync, peer access enabled where the link allows; all destinations are in flight together,
 * one stream per destination).  devices[i] may be the root's own device (a plain copy).  Each replica is an
 * ordinary index: search it with its own contexts, free it with idist_index_free.  On error nothing is left
 * allocated.  (The multi-PROCESS flavour — one rank per GPU, RCCL broadcast into idist_index_alloc'ed
 * replicas through idist_index_device_buffers — is instant-distance_amd/dist.py.) */
idist_status idist_replicate(const idist_index* root, const int32_t* devices, uint32_t n_devices,
                             idist_index** replicas);
/* The same replication as ONE RCCL broadcast per buffer (points, zero, upper) over a single-process communicator
 * (ncclCommInitAll over the root's device and the distinct destination devices, ncclBroadcast inside one group,
 * one stream per device): RCCL picks the ring / tree over xGMI instead of the root feeding every peer itself.
 * librccl.so is loaded on first use (dlopen; IDIST_ERR_UNSUPPORTED if it is missing).  A destination on the root's
 * own device is served inside the same broadcast (recvbuff != sendbuff on the root rank).  *seconds (optional):
 * wall time of the broadcasts, communicator set-up excluded. */
idist_status idist_replicate_rccl(const idist_index* root, const int32_t* devices, uint32_t n_devices,
                                  idist_index** replicas, double* seconds);
/* Hnsw::search for nq host queries over n_shards (replica, context) pairs: the queries are cut into the
 * contiguous ranges [nq*i/n_shards, nq*(i+1)/n_shards) — what a caller partitioning over threads does —
 * each searched by idist_search_batch on its own GPU from its own host thread, results written to the same
 * ranges of the outputs.  No collective, no device-to-device traffic; the result is identical to one
 * idist_search_batch over the whole batch. */
idist_status idist_search_batch_sharded(const idist_index* const* replicas, idist_search_ctx* const* ctxs,
                                        uint32_t n_shards, const float* queries, uint32_t nq,
                                        uint32_t* out_pid, float* out_dist, uint32_t* out_count,
                                        uint32_t* out_counters);

/* ---- partitioned index: several indexes searched as one ------------------------ */
/* The reference has one `Hnsw` per set of points.  A partitioned index is an ordered list of 1..64 ordinary indexes
 * ("parts") with the same dim, metric and ef_search, on any devices: an index larger than one GPU's memory, built on several
 * GPUs side by side.  ("Partitioned", not "sharded": sharded above means QUERIES split over replicas of one index.)
 *   global id of a point = base[p] + its PointId inside part p, base[p] = points in parts 0..p-1;
 *   search of one query  = Hnsw::search (core/lib.rs:352-383) on every part, ids made global, the lists merged by the
 *                          reference's `Candidate` order (core/types.rs:229-234: distance, then id), the first ef_search kept;
 *                          count = min(ef_search, sum of the parts' counts); counters = the parts' counters summed.
 * One part is the identity: the arrays idist_search_batch returns for that part.  Empty parts contribute nothing.
 *
 * idist_merge_topk_device is that merge on its own: n_lists (1..64) sorted lists per query, d_pid / d_dist
 * [n_lists][nq][width], d_count [n_lists][nq], d_counters [n_lists][nq][3] (may be NULL), all in the memory of `device`;
 * list l's ids are offset by base[l] (HOST array of n_lists entries, read before the call returns).  Output as
 * idist_search_batch_device writes it with ef_search = out_width: d_out_pid / d_out_dist [nq][out_width] padded with
 * IDIST_INVALID / +inf, d_out_count [nq], d_out_counters [nq][3] (may be NULL).  width, out_width: 1..IDIST_MAX_EF.  Only the
 * first min(count, width) entries of a list are read as results — whatever lies behind them is ignored.  Distances must be
 * what the engine produces (non-negative, one NaN pattern): they are ordered by their bit patterns.  Enqueued on
 * `hip_stream` (a hipStream_t, may be NULL) without synchronising. */
idist_status idist_merge_topk_device(const void* d_pid, const void* d_dist, const void* d_count,
                                     const void* d_counters, uint32_t n_lists, uint32_t nq, uint32_t width,
                                     const uint32_t* base, uint32_t out_width, void* d_out_pid, void* d_out_dist,
                                     void* d_out_count, void* d_out_counters, int32_t device, void* hip_stream);

typedef struct idist_partitioned idist_partitioned;
typedef struct idist_partitioned_info {
    uint32_t n_parts, dim, ef_search;
    int32_t metric;
    int32_t merge_device;       /* the device of part 0: the parts' lists meet and are merged there */
    uint64_t n;                 /* points in all parts */
    uint32_t base[65];          /* base[p] = first global id of part p; base[n_parts] = n */
} idist_partitioned_info;
/* The parts are BORROWED: the caller keeps every index alive until idist_partitioned_free and frees it afterwards.  The
 * object is one `&mut Search` over all parts (core/lib.rs:352-356): it owns a search context and a stream per part and
 * the staging memory of the merge, and is used by one thread at a time.  IDIST_ERR_INVALID_ARG (naming the part) when
 * n_parts is 0 or above 64, a part is NULL, dim / metric / ef_search differ, or the points together do not fit a PointId. */
idist_status idist_partitioned_new(const idist_index* const* parts, uint32_t n_parts, idist_partitioned** out);
void idist_partitioned_free(idist_partitioned* p);
idist_status idist_partitioned_get_info(const idist_partitioned* p, idist_partitioned_info* out);
/* Hnsw::search over all parts for nq host queries; shapes and padding exactly as idist_search_batch, ids global.  The queries
 * are uploaded once per distinct device, every part is searched on its own stream (idist_search_batch_device) straight into
 * its slice of the staging memory on the merge device (parts elsewhere: into memory of their own device, then one peer copy),
 * one merge kernel, results to the host.  Blocks until done.  Strict ties: a part whose tie region overflowed is searched
 * again with the larger region, as idist_search_batch does — IDIST_ERR_TIE_OVERFLOW never reaches the caller.  The parts'
 * dim / metric / ef_search are compared again at every call (idist_index_set_ef_search may have changed one). */
idist_status idist_partitioned_search_batch(idist_partitioned* p, const float* queries, uint32_t nq,
                                            uint32_t* out_pid, float* out_dist, uint32_t* out_count,
                                            uint32_t* out_counters);
/* Exact k nearest neighbours over all parts: the same merge, width k, over every part's idist_bruteforce (part p contributes
 * min(k, n_p) items) — the brute-force check of tests/all.rs:60-67 on the points concatenated in global-id order, ties
 * (distance, then id) included.  out_pid / out_dist: nq*k, padded with IDIST_INVALID / +inf when fewer than k points exist. */
idist_status idist_partitioned_bruteforce(idist_partitioned* p, const float* queries, uint32_t nq, uint32_t k,
                                          uint32_t* out_pid, float* out_dist);
/* HIP-event duration of the last merge kernel launched through p, milliseconds. */
idist_status idist_partitioned_last_merge_ms(idist_partitioned* p, float* ms);
/* ms[i] = HIP-event duration of part i's last search kernel (idist_search_ctx_last_kernel_ms of the context p owns for it),
 * milliseconds; 0 for an empty part, -1 where no launch was timed.  *n_out = entries written (<= cap): what the merge's
 * own time is set against. */
idist_status idist_partitioned_last_search_kernel_ms(idist_partitioned* p, float* ms, uint32_t cap, uint32_t* n_out);

/* ---- restricted search: the k nearest among an allowed subset --------------------------------------- */
/* DEFINED through what is already exact: Hnsw::search (core/lib.rs:352-383) at growing ef_search, filtered, and an exact scan of the
 * allowed rows below a derivable selectivity and when the ladder ends.  The walk itself is not touched.
 *   A          the allowed set, a bitmap of (n + 31) / 32 u32 words: point `pid` is allowed iff bit pid % 32 of word pid / 32 is set;
 *              bits at positions >= n are ignored.  One set per call, shared by the batch (several: idist_search_batch_allowed_sets).
 *   k          1 <= k <= ef_search of the index.
 *   ladder     E[0] = ef_search, E[r + 1] = min(4 * E[r], IDIST_MAX_EF); it ends with the rung that equals IDIST_MAX_EF
 *              (ef_search = 100: 100, 400, 1600, 4096).
 *   max_rungs  -1: the whole ladder; m >= 0: only rungs r < m; 0: no rung at all = a restricted brute force (the ground truth for
 *              recall).
 * For one query:
 *   1. n == 0, ef_search == 0 or |A| == 0: count 0, rung IDIST_RUNG_NONE.
 *   2. |A| <= k: exact (step 5).
 *   3. The start rung r0 is the first permitted r with E[r] * |A| >= k * n (64-bit integers): a rung whose expected number of
 *      allowed hits is below k is not tried.  No such r: exact.
 *   4. For r = r0, r0 + 1, ... among the permitted rungs: L = the result of Hnsw::search at ef_search = E[r] — for every metric the
 *      raw distances of the stored rows, what idist_search_batch produces before its report pass.  At least k entries of L allowed:
 *      the answer is the first k allowed entries of L, in L's order; rung = r; stop.
 *   5. Exact: the k nearest points of A by the canonical distance, ordered by (distance, id) — idist_bruteforce restricted to A;
 *      count = min(k, |A|); rung IDIST_RUNG_EXACT.
 * Every query so gets exactly min(k, |A|) results.  Distances go through the metric's report once, at the end, on the [nq][k] result
 * (as idist_partitioned_search_batch does); padding is IDIST_INVALID / +inf.  out_counters (optional, nq*3): {n_dist, n_exp0,
 * n_expU} summed over the rungs that query actually ran; the exact step adds nothing to them (it shows in the rung).  A later rung
 * whose ef_search does not fit a wave's LDS ends the ladder there as max_rungs would; the same failure at rung 0 is returned, as
 * idist_search_batch returns it.  Strict ties: a rung whose tie region overflowed is searched again, IDIST_ERR_TIE_OVERFLOW never
 * reaches the caller.  IDIST_ERR_INVALID_ARG: k out of range, max_rungs < -1, null pointers.
 * Host pointers; blocks until done.  The call uses ctx as one `&mut Search` (its stream, its slots, staging memory the context owns
 * and frees); idx stays shared and is never mutated — the rungs carry their own ef_search.  Staging: the widest rung holds
 * 8 * E[r] bytes per query still pending.
 * Cost: a query that climbs the whole ladder costs about 1.3 searches at ef_search 4096 (the rungs below add a quarter, a
 * sixteenth, ...) plus a scan of A; max_rungs is the caller's bound.
 * Out of scope: device-pointer / stream variants and idist_search_batch_sharded.  Several sets in one call:
 * idist_search_batch_allowed_sets below; the partitioned index: idist_partitioned_search_batch_allowed_sets. */
#define IDIST_RUNG_NONE  254u
#define IDIST_RUNG_EXACT 255u
idist_status idist_search_batch_allowed(const idist_index* idx, idist_search_ctx* ctx, const float* queries, uint32_t nq,
                                        const uint32_t* allow_bits, uint32_t k, int32_t max_rungs,
                                        uint32_t* out_pid, float* out_dist,      /* nq*k */
                                        uint32_t* out_count, uint32_t* out_rung, /* nq; out_rung may be NULL */
                                        uint32_t* out_counters);                 /* nq*3 or NULL */
/* Several allowed sets per call, one per query: tenants, ACL groups, categories and date ranges mixed in one batch.
 *   allow_bits  n_sets bitmaps of (n + 31) / 32 words each, one after the other, each as in idist_search_batch_allowed; bits at
 *               positions >= n of every set are ignored.  The buffer is neither written nor copied on the host to clean it.
 *   n_sets      >= 1.
 *   set_of      [nq]: query q is restricted to set set_of[q] (< n_sets).  NULL: query q uses set q, and n_sets must equal nq.
 * DEFINITION: row q of every output is row 0 of
 *   idist_search_batch_allowed(idx, ctx, &queries[q * dim], 1, allow_bits + set_of[q] * ((n + 31) / 32), k, max_rungs, ...)
 * — ids, order, distance bits, count, rung and counters.  Nothing else is new: the ladder, the start rule, the exact step, the
 * metric's report on the final [nq][k] result, the padding, the strict-tie retry and max_rungs are the single-set call's.  Every
 * query evaluates the start rule E[r] * |A| >= k * n with its own set's size, so the queries of one call may start on different
 * rungs: a query waits, unlaunched, until its start rung comes up, and its counters sum only the rungs it ran.  A later rung that
 * does not fit a wave's LDS ends the ladder for every query still waiting or pending (they are answered exactly); the same failure
 * on rung 0 is returned.  The call fails whenever one of those single-set calls would fail.
 * IDIST_ERR_INVALID_ARG: n_sets == 0; set_of == NULL with n_sets != nq; a set_of[q] >= n_sets (the message names q); k out of range,
 * max_rungs < -1, null pointers.
 * The sets' sizes and start rungs are counted on the device; the exact step reads the bitmaps themselves (no id list is made, the
 * staging does not grow with n_sets beyond the n_sets * ((n + 31) / 32) * 4 bytes of the bitmaps): n / 8 bytes of bitmap per
 * (pending query, call) on top of the allowed rows.
 * Host pointers; blocks until done; ctx is the `&mut Search`, idx is never mutated — as the single-set call.
 * Out of scope: device-pointer / stream variants and idist_search_batch_sharded.  The partitioned index:
 * idist_partitioned_search_batch_allowed_sets below. */
idist_status idist_search_batch_allowed_sets(const idist_index* idx, idist_search_ctx* ctx, const float* queries, uint32_t nq,
                                             const uint32_t* allow_bits,              /* [n_sets][(n + 31) / 32] */
                                             uint32_t n_sets, const uint32_t* set_of, /* [nq] or NULL */
                                             uint32_t k, int32_t max_rungs,
                                             uint32_t* out_pid, float* out_dist,      /* nq*k */
                                             uint32_t* out_count, uint32_t* out_rung, /* nq; out_rung may be NULL */
                                             uint32_t* out_counters);                 /* nq*3 or NULL */
/* Restricted search over a partitioned index, one allowed set per query: the two exact things above, composed.
 *   allow_bits  n_sets bitmaps over the GLOBAL ids: (N + 31) / 32 words each, N = the points in all parts, bit g = global id g; bits at
 *               positions >= N are ignored.  The buffer is neither written nor copied on the host to clean it.
 *   set_of      as in idist_search_batch_allowed_sets.
 * DEFINITION: A_p = the slice of query q's set that falls into part p (bit i of A_p = bit base[p] + i of the set, i < n_p).  Row q is the
 * merge of the P lists
 *   idist_search_batch_allowed(part p, ctx, &queries[q * dim], 1, A_p, k, max_rungs, ...)      raw distances, ids + base[p]
 * by the reference's `Candidate` order (distance bits, then global id), the first k kept — the merge of
 * idist_partitioned_search_batch at width k.  So:
 *   - every part runs its own ladder with its own start rule on |A_p| and n_p: a part that holds none of a query's allowed points
 *     answers IDIST_RUNG_NONE at once, one where they are rare goes straight to the exact scan (range- or tenant-partitioned data);
 *   - count = min(k, sum over p of min(k, |A_p|)) = min(k, |A|), the guarantee of the single-index call;
 *   - out_counters = the parts' counters summed; out_rung[q * n_parts + p] = part p's rung for query q (IDIST_RUNG_NONE for an empty
 *     part or an empty slice);
 *   - the metric's report runs once, after the merge, on the [nq][k] result; padding is IDIST_INVALID / +inf;
 *   - IDIST_ERR_TIE_OVERFLOW never reaches the caller; a part's failure on rung 0 (a wave's LDS) is returned, the message prefixed
 *     "part <p> (device <d>): " as idist_partitioned_search_batch does;
 *   - 1 <= k <= ef_search; N == 0 or ef_search == 0: every count 0, every rung IDIST_RUNG_NONE, every counter 0.
 * One part is the identity: every output equals idist_search_batch_allowed_sets on that part.
 * IDIST_ERR_INVALID_ARG: the cases of idist_search_batch_allowed_sets; the parts' dim / metric / ef_search are compared again at every
 * call.  Every part finds k of its own although the union needs only k (as every part of idist_partitioned_search_batch returns
 * ef_search): the price of a definition that composes two exact things.
 * The queries and set_of are uploaded once per distinct device; of the bitmaps every part's device receives the words that hold the
 * part's bits (one strided copy: the bitmaps' size in total, plus at most one word per set and part) and cuts its own bitmaps out of
 * them on the device (idist_allowed_slice_device's kernel).  The ladders block on the host once per rung, so the parts run side by
 * side, one host thread per non-empty part for the duration of the call.  Host pointers; blocks until done; p is used by one thread
 * at a time.  Out of scope: device-pointer / stream variants and idist_search_batch_sharded. */
idist_status idist_partitioned_search_batch_allowed_sets(idist_partitioned* p, const float* queries, uint32_t nq,
                                                         const uint32_t* allow_bits,              /* [n_sets][(N + 31) / 32] */
                                                         uint32_t n_sets, const uint32_t* set_of, /* [nq] or NULL */
                                                         uint32_t k, int32_t max_rungs,
                                                         uint32_t* out_pid, float* out_dist,      /* nq*k, global ids */
                                                         uint32_t* out_count,                     /* nq */
                                                         uint32_t* out_rung,                      /* [nq][n_parts] or NULL */
                                                         uint32_t* out_counters);                 /* nq*3 or NULL */
/* Host time (ms) the last idist_partitioned_search_batch_allowed_sets or idist_partitioned_search_batch_range_allowed_sets through p
 * spent on the bitmaps: the strided uploads and the slice kernels of all parts (waited for, to be timed, unless
 * IDIST_KERNEL_EVENTS=0).  After an attribute call (idist_partitioned_search_batch_attr / _range_attr): the HIP-event durations of the
 * parts' bitmap kernels, summed, instead.  0 before the first call. */
idist_status idist_partitioned_last_allowed_slice_ms(idist_partitioned* p, float* ms);
/* The slice on its own: d_bits holds n_sets rows of pitch_words u32 words, d_out n_sets rows of (n_out + 31) / 32 words, both in the
 * memory of `device`.  out[s] bit i = in[s] bit bit_offset + i for i < n_out; the bits at positions >= n_out of a row's last word are
 * written as 0.  No source word at or beyond (bit_offset + n_out + 31) / 32 of a row is read: the source may end exactly there
 * (a smaller pitch_words is IDIST_ERR_INVALID_ARG).  n_out == 0 or n_sets == 0: nothing is done.  Enqueued on `hip_stream` (a
 * hipStream_t, may be NULL) without synchronising, as idist_merge_topk_device. */
idist_status idist_allowed_slice_device(const void* d_bits, uint32_t n_sets, uint32_t pitch_words, uint64_t bit_offset,
                                        uint32_t n_out, void* d_out, int32_t device, void* hip_stream);
/* HIP-event durations (ms) of the kernels the last idist_search_batch_allowed / idist_search_batch_allowed_sets through ctx ran
 * around its searches, summed over its rungs: the select passes (and the several-sets call's count pass), the pending-list passes,
 * the exact step (scan + merge).  0 with IDIST_KERNEL_EVENTS=0.  The rungs' own search kernels are in idist_search_ctx_kernel_times. */
idist_status idist_search_ctx_allowed_kernel_ms(idist_search_ctx* ctx, float* select_ms, float* pending_ms, float* exact_ms);

/* ---- range search: every point within a radius ------------------------------------------------------- */
/* Defined, as the restricted search is, through Hnsw::search at growing ef_search and an exact scan where that ladder ends.  The
 * walk itself is not touched.
 *   radius     one f32 for the batch (n_radius == 1) or one per query (n_radius == nq).  NaN is IDIST_ERR_INVALID_ARG (the message
 *              names the query); +inf, 0, -0.0 and negative radii are legal (IDIST_METRIC_DOT reports about -q.x).
 *   max_rungs  as in idist_search_batch_allowed: -1 the whole ladder, m >= 0 only the rungs r < m, 0 the exact scan alone (the
 *              ground truth for recall).  The ladder is that call's: E[0] = ef_search, E[r + 1] = min(4 * E[r], IDIST_MAX_EF).
 *   within     point x is within the radius of query q iff report(d) <= r_q as an f32 comparison: d the RAW canonical distance of the
 *              stored row (what idist_search_batch holds before its report pass), report the metric's: the identity for L2SQ and L2,
 *              0.5f * d for cosine, 0.5f * (d - (s(q) + S)) for DOT with +inf and NaN reported unchanged.  A NaN distance is never
 *              within.  report is non-decreasing in d (every float step is monotone), so the entries of a sorted list that are
 *              within are a prefix of it.
 * For one query:
 *   1. n == 0 or ef_search == 0: count 0, rung IDIST_RUNG_NONE.
 *   2. For r = 0, 1, ... among the permitted rungs: L = the result of Hnsw::search at ef_search = E[r], c entries.  c == E[r] and
 *      every entry within: the list is saturated, the next rung runs.  Otherwise the answer is the prefix of L that is within, in L's
 *      order; rung = r; stop (a count of 0 is an answer).
 *   3. The ladder ended saturated, or max_rungs == 0: exact — every point within the radius, ordered by (raw distance bits, id);
 *      rung IDIST_RUNG_EXACT.
 *   4. Reported distances are report(d), applied once, at the end.
 *   5. out_counters sums {n_dist, n_exp0, n_expU} over the rungs the query ran; the exact step adds nothing.
 * A later rung that does not fit a wave's LDS ends the ladder as max_rungs would (on rung 0 the failure is returned), and a strict-tie
 * overflow is retried and never reaches the caller, as in idist_search_batch_allowed.  What a rung returns for a query does not depend
 * on who else is pending: every row of the batch is what the call returns for that query alone.
 *   out_lims   [nq + 1], lims[0] = 0: query q owns the entries [lims[q], lims[q + 1]) of the flat pid / distance arrays
 *              idist_search_ctx_range_fetch hands out.  out_rung [nq], out_counters [nq][3]: may be NULL.
 *   max_total  the caller's bound on lims[nq].  When the results known after a step (a rung, the exact step) exceed it the call returns
 *              IDIST_ERR_INVALID_ARG — the message says how many were known by then — and the context holds no results: nothing is
 *              truncated silently.
 * Host pointers; the call blocks until done.  ctx is the `&mut Search`: it owns the staging and keeps the results until the next
 * range call or until they are fetched; idx is never mutated.  nq == 0: lims[0] = 0. */
idist_status idist_search_batch_range(const idist_index* idx, idist_search_ctx* ctx, const float* queries, uint32_t nq,
                                      const float* radius, uint32_t n_radius, int32_t max_rungs, uint64_t max_total,
                                      uint64_t* out_lims, uint32_t* out_rung, uint32_t* out_counters);
/* The results of the last successful idist_search_batch_range, idist_search_batch_range_allowed_sets or idist_search_batch_range_attr
 * through ctx: out_pid / out_dist [lims[nq]] each (may be NULL when that is 0), in query order, reported distances.  They are handed
 * out once: a fetch without a preceding successful range call (or a second one) is IDIST_ERR_INVALID_ARG. */
idist_status idist_search_ctx_range_fetch(idist_search_ctx* ctx, uint32_t* out_pid, float* out_dist);
/* HIP-event durations (ms) of the kernels the last idist_search_batch_range or idist_search_batch_range_allowed_sets through ctx ran
 * around its searches: the select passes (limits, within-prefixes, offsets, copies, pending lists; the restricted call's count pass),
 * the exact step's two scans with their offsets, the sort.  0 with IDIST_KERNEL_EVENTS=0.  The rungs' own search kernels are in
 * idist_search_ctx_kernel_times. */
idist_status idist_search_ctx_range_kernel_ms(idist_search_ctx* ctx, float* select_ms, float* scan_ms, float* sort_ms);

/* ---- restricted range search: every point of an allowed set within a radius ------------------------------ */
/* The composition of the two calls above, one allowed set per query: "every point of my subset within a radius".  Defined through
 * what is already exact, as they are.
 *   radius, n_radius, max_rungs, max_total   exactly as idist_search_batch_range.  A NaN radius is IDIST_ERR_INVALID_ARG and the message
 *               names the query.
 *   allow_bits, n_sets, set_of               exactly as idist_search_batch_allowed_sets: n_sets bitmaps of (n + 31) / 32 words each;
 *               bits at positions >= n are ignored; set_of == NULL requires n_sets == nq; the buffer is neither written nor cleaned
 *               on the host.
 *   within      idist_search_batch_range's: report(d) <= r_q on the raw canonical distance.
 *   the ladder  E[0] = ef_search, E[r + 1] = min(4 * E[r], IDIST_MAX_EF).
 * For one query q with A = its own set:
 *   1. Nothing to find.  n == 0, ef_search == 0 or |A| == 0: count 0, rung IDIST_RUNG_NONE.
 *   2. End rule (per query).  Rung r is permitted for q iff max_rungs permits it and E[r] < 2 * |A|, in 64-bit integers: the exact step
 *      below measures each of A's rows twice, 2 |A| row reads, while a search at E[r] fills a list of E[r] entries and measures at
 *      least that many rows.  E is increasing, so the permitted rungs are a prefix r < R_q; R_q == 0 sends the query straight to 4.
 *   3. Rungs.  For r = 0, 1, ... < R_q: L = the result of Hnsw::search at ef_search = E[r], c entries, pre the length of its
 *      within-prefix.  c == E[r] and pre == c: saturated — judged on the unrestricted list, as in idist_search_batch_range — the next
 *      rung runs.  Otherwise the answer is the allowed entries of L[0:pre], in L's order; rung = r (a count of 0 is an answer).
 *   4. Exact.  The query is still unanswered after its last permitted rung, or R_q == 0: every point of A within the radius, ordered by
 *      (raw distance bits, id); rung IDIST_RUNG_EXACT.
 *   5. Reported distances are report(d), applied once, at the fetch.  out_counters sums {n_dist, n_exp0, n_expU} over the rungs the
 *      query ran; the exact step adds nothing.
 * As in idist_search_batch_range: a later rung that does not fit a wave's LDS ends the ladder for every query still pending (on rung 0
 * the failure is returned); a strict-tie overflow is retried and never reaches the caller; every row of the batch is what the call
 * returns for that query alone; max_total bounds the RESTRICTED total known after each step, with that call's message, and nothing is
 * truncated.  So: row q's ids are idist_search_batch_range's answer of the same rung filtered by A whenever that rung is permitted;
 * with max_rungs == 0 the answer is the exhaustive one; with every bit set and 2 n > IDIST_MAX_EF every output equals
 * idist_search_batch_range's.
 * The sets' sizes and last rungs are counted on the device; the exact step reads the bitmaps themselves and fetches only allowed rows
 * (no id list is made; the staging does not grow beyond the bitmaps' own bytes).
 * Host pointers; the call blocks until done.  ctx is the `&mut Search`: it holds the results exactly as after
 * idist_search_batch_range — idist_search_ctx_range_fetch hands them out once, idist_search_ctx_range_kernel_ms reports the three
 * times; idx is never mutated.  nq == 0: lims[0] = 0.
 * IDIST_ERR_INVALID_ARG: the cases of idist_search_batch_range and of idist_search_batch_allowed_sets' sets (n_sets == 0; set_of == NULL
 * with n_sets != nq; a set_of[q] >= n_sets, the message names q); null pointers.
 * Out of scope: device-pointer / stream variants and idist_search_batch_sharded.  The partitioned index:
 * idist_partitioned_search_batch_range_allowed_sets below. */
idist_status idist_search_batch_range_allowed_sets(const idist_index* idx, idist_search_ctx* ctx, const float* queries, uint32_t nq,
                                                   const float* radius, uint32_t n_radius,
                                                   const uint32_t* allow_bits,              /* [n_sets][(n + 31) / 32] */
                                                   uint32_t n_sets, const uint32_t* set_of, /* [nq] or NULL */
                                                   int32_t max_rungs, uint64_t max_total,
                                                   uint64_t* out_lims, uint32_t* out_rung, uint32_t* out_counters);

/* Range search over a partitioned index: the range search above on every part, merged on the device.
 * DEFINITION: row q is the merge, by the u64 key  raw distance bits << 32 | global id, of what idist_search_batch_range returns for
 * query q on every non-empty part, global id = base[p] + PointId.  Every part gets the same radius[q] and the same max_rungs.  So:
 *   - every part climbs its own ladder and ends in its own exact scan, as in idist_partitioned_search_batch_allowed_sets; a part's
 *     list is already ascending in that key and keys of different parts are distinct; "within" is the definition above, unchanged,
 *     decided by the parts;
 *   - reported distances are report(d) of the merged raw distances, applied once, after the merge, with that query's own term (DOT:
 *     s(q) + S, every part holds the same S): the bits equal what the single index reports for the same raw distance;
 *   - out_lims [nq + 1], lims[0] = 0: query q owns [lims[q], lims[q + 1]) of the flat pid (GLOBAL ids) and distance arrays
 *     idist_partitioned_range_fetch hands out, nearest first;
 *   - out_rung[q * n_parts + p] = part p's rung for query q, IDIST_RUNG_NONE for an empty part; out_counters = the parts' counters
 *     summed (both may be NULL);
 *   - max_total bounds the merged total lims[nq]; every part is given the same bound (its own total can never legitimately exceed
 *     it) and the merged total is checked again.  Beyond it: IDIST_ERR_INVALID_ARG, the message says how many results were known
 *     (a part's message is prefixed "part <p> (device <d>): "), and no results are held;
 *   - a NaN radius is IDIST_ERR_INVALID_ARG with the query named; nq == 0: lims[0] = 0; no points at all, or ef_search == 0: every count
 *     0, every rung IDIST_RUNG_NONE, every counter 0;
 *   - IDIST_ERR_TIE_OVERFLOW never reaches the caller; a part's failure on rung 0 is returned with the prefix above.
 * With max_rungs == 0 the answer is every point of the whole set within the radius, ordered by (raw distance bits, global id): what
 * one exact scan over all rows gives.  One part is the identity: every output equals idist_search_batch_range on that part.
 * The queries are uploaded once per distinct device; the parts' searches block on the host once per rung, so the parts run side by
 * side, one host thread per non-empty part for the duration of the call.  The merge reads the lists of the parts on the merge device
 * where their contexts hold them (completion order, a per-query offset and count); parts elsewhere send keys, offsets and counts by
 * peer copies.  Work is divided by results, not by queries; up to 64 lists; no size cap but max_total.  ONE read-back of the merged
 * total precedes the merge.  The results are held by p until the next range call through it or until they are fetched.
 * Host pointers; blocks until done; p is used by one thread at a time.  Out of scope: device-pointer / stream variants and
 * idist_search_batch_sharded.  Restricted to one allowed set per query: idist_partitioned_search_batch_range_allowed_sets below. */
idist_status idist_partitioned_search_batch_range(idist_partitioned* p, const float* queries, uint32_t nq,
                                                  const float* radius, uint32_t n_radius, int32_t max_rungs, uint64_t max_total,
                                                  uint64_t* out_lims,        /* nq + 1 */
                                                  uint32_t* out_rung,        /* [nq][n_parts] or NULL */
                                                  uint32_t* out_counters);   /* nq*3 or NULL */
/* Restricted range search over a partitioned index: the two calls above, composed (DESIGN.md sections 4.10 and 8.1).
 *   allow_bits, n_sets, set_of   exactly as idist_partitioned_search_batch_allowed_sets: n_sets bitmaps over the GLOBAL ids, (N + 31) / 32
 *                                words each, bits at positions >= N ignored, the buffer neither written nor cleaned on the host;
 *                                set_of == NULL requires n_sets == nq.
 *   radius, n_radius, max_rungs, max_total, out_lims, out_rung, out_counters   exactly as idist_partitioned_search_batch_range.
 * DEFINITION: A_p = the slice of query q's set that falls into part p (bit i of A_p = bit base[p] + i of the set, i < n_p).  Row q is the
 * merge, by the u64 key  raw distance bits << 32 | global id, of what
 *   idist_search_batch_range_allowed_sets(part p, ctx, &queries[q * dim], 1, &radius[q], 1, A_p, 1, NULL, max_rungs, ...)
 * returns on every non-empty part.  So:
 *   - every part applies its own end rule E[r] < 2 |A_p|, climbs its own ladder and ends in its own exact scan of A_p's rows; a part
 *     that holds none of a query's allowed points answers IDIST_RUNG_NONE at once;
 *   - the metric's report runs once, after the merge, with the query's own term;
 *   - max_total bounds the merged RESTRICTED total: it is passed to every part and checked again after the merge, with the messages
 *     and the "holds nothing" rule of idist_partitioned_search_batch_range;
 *   - the results are held by p and handed out once by idist_partitioned_range_fetch; idist_partitioned_last_range_merge_ms and
 *     idist_partitioned_last_allowed_slice_ms report the merge and the bitmaps' upload + slice;
 *   - with max_rungs == 0 the answer is every allowed point within the radius, ordered by (raw distance bits, global id).
 * One part is the identity: every output equals idist_search_batch_range_allowed_sets on that part.  With every bit set and
 * 2 n_p > IDIST_MAX_EF in every part, every output equals idist_partitioned_search_batch_range's.
 * IDIST_ERR_INVALID_ARG: the cases of idist_partitioned_search_batch_range and of idist_search_batch_allowed_sets' sets.
 * The bitmaps reach the parts as in idist_partitioned_search_batch_allowed_sets (one strided copy + the slice kernel per part);
 * everything else is idist_partitioned_search_batch_range's schedule, which the plain call still launches unchanged.
 * Host pointers; blocks until done; p is used by one thread at a time.  Out of scope: device-pointer / stream variants and
 * idist_search_batch_sharded. */
idist_status idist_partitioned_search_batch_range_allowed_sets(idist_partitioned* p, const float* queries, uint32_t nq,
                                                               const float* radius, uint32_t n_radius,
                                                               const uint32_t* allow_bits,              /* [n_sets][(N + 31) / 32], global ids */
                                                               uint32_t n_sets, const uint32_t* set_of, /* [nq] or NULL */
                                                               int32_t max_rungs, uint64_t max_total,
                                                               uint64_t* out_lims,        /* nq + 1 */
                                                               uint32_t* out_rung,        /* [nq][n_parts] or NULL */
                                                               uint32_t* out_counters);   /* nq*3 or NULL */
/* The results of the last successful idist_partitioned_search_batch_range, idist_partitioned_search_batch_range_allowed_sets or
 * idist_partitioned_search_batch_range_attr through p: out_pid (global ids) / out_dist [lims[nq]] each
 * (may be NULL when that is 0).  The rules of idist_search_ctx_range_fetch: handed out once; a second fetch, or one with nothing held,
 * is IDIST_ERR_INVALID_ARG. */
idist_status idist_partitioned_range_fetch(idist_partitioned* p, uint32_t* out_pid, float* out_dist);
/* HIP-event duration (ms) of the counts, prefix-sum and merge kernels of the last idist_partitioned_search_batch_range through p
 * (0 when it had nothing to find); IDIST_ERR_INVALID_ARG before the first one.  The parts' own kernels:
 * idist_partitioned_last_search_kernel_ms. */
idist_status idist_partitioned_last_range_merge_ms(idist_partitioned* p, float* ms);
/* The counts and merge kernels behind it on their own, on caller-made lists in the memory of `device` (the role
 * idist_merge_topk_device plays for the top-k merge).  d_keys / d_off / d_cnt: HOST arrays of n_lists (1..64) device pointers.  List l
 * holds for query q the d_cnt[l][q] (u32) keys  raw distance bits << 32 | local id  (u64) at d_keys[l] + d_off[l][q] (u64 offsets, in
 * keys, in any order of the queries), ascending; its global ids are base[l] + local id (< 2^32 - 1), so that the keys of different
 * lists are distinct.  The counts rule: nothing beyond a list's count is read, and a list that is empty for every query may have a
 * NULL d_keys[l].  d_lims [nq + 1] (u64) receives the prefix sum of the merged counts, *out_total its last entry; d_out_pid /
 * d_out_dist [capacity]: query q's merged keys at [lims[q], lims[q + 1]) as global ids and as report(d) for `metric` (IDIST_METRIC_DOT:
 * d_sq [nq] holds s(q), dot_bound is S; else d_sq may be NULL).  *out_total > capacity: IDIST_ERR_INVALID_ARG and nothing is written
 * to the output arrays; nothing is ever written beyond lims[nq].  The call waits for `hip_stream` (a hipStream_t, may be NULL) once,
 * to read the total back; the merge itself is enqueued without synchronising. */
idist_status idist_range_merge_device(const void* const* d_keys, const void* const* d_off, const void* const* d_cnt,
                                      uint32_t n_lists, uint32_t nq, const uint32_t* base, int32_t metric, const void* d_sq,
                                      float dot_bound, uint64_t capacity, void* d_lims, void* d_out_pid, void* d_out_dist,
                                      uint64_t* out_total, int32_t device, void* hip_stream);

/* ---- attribute filters: a u32 per point, an interval per query, the bitmaps made on the device -------------- */
/* The allowed sets above are for "tenants, ACL groups, categories and date ranges mixed in one batch": the caller holds one small
 * integer per point and one condition per query.  An idist_attr keeps that integer on the device, next to the rows; the four calls
 * below take an interval per query instead of bitmaps and make the bitmaps where they are read.
 *   values      one u32 per point: PointId order for an index, global-id order (N of them) for a partitioned index.
 *   an attr     a device copy of the values — on the index's device; for a partitioned index every non-empty part's slice
 *               values[base[p] .. base[p] + n_p) on that part's own device.  Immutable after creation, may be shared by any number of
 *               threads and contexts.  Bound to the handle it was made for by identity, not by address, as a search context is: with any
 *               other index or partitioned index, with an index's attribute in a partitioned call or the reverse, every call below is
 *               IDIST_ERR_INVALID_ARG.  The index is not touched and stays immutable.  n == 0 is legal (values may be NULL).  Free it
 *               with idist_attr_free, before or after the handle it was made for.
 *   lo, hi      n_cond intervals: point i satisfies interval c iff lo[c] <= values[i] && values[i] <= hi[c], UNSIGNED comparisons
 *               (lo == hi: equality; lo > hi: the empty set, legal; (0, 0xFFFFFFFF): every point).
 *   n_cond      1: one condition for the whole batch; nq: one per query — as n_radius.  Anything else is IDIST_ERR_INVALID_ARG.
 * DEFINITION: let D be the distinct (lo, hi) pairs of the call, bits[s] the bitmap of pair s (bit i = the condition on values[i], the
 * bits at positions >= n zero) and set_of[q] the index of query q's pair.  Every output of a call below equals, bit for bit, the output
 * of the call it is listed with, given (bits, |D|, set_of):
 *   idist_search_batch_attr                     idist_search_batch_allowed_sets
 *   idist_search_batch_range_attr               idist_search_batch_range_allowed_sets       (results: idist_search_ctx_range_fetch)
 *   idist_partitioned_search_batch_attr         idist_partitioned_search_batch_allowed_sets, bitmaps over the global ids
 *   idist_partitioned_search_batch_range_attr   idist_partitioned_search_batch_range_allowed_sets  (idist_partitioned_range_fetch)
 * and everything else comes from those calls: the other arguments and their errors (a NaN radius names its query), the trivial cases
 * (nq == 0, no points, ef_search == 0), max_total, the strict-tie retry, the LDS rule for later rungs, out_rung [nq][n_parts] for the
 * parts.  Null lo / hi / attr: IDIST_ERR_INVALID_ARG.
 * The conditions are grouped on the host (nq entries); lo / hi / set_of are uploaded; one kernel on the context's stream writes the
 * |D| bitmaps where the restricted search reads them, and the call goes on exactly as the bitmap call does.  On a partitioned index
 * every part makes its own bitmaps from its own slice of the values, on its own stream: no strided upload, no slice kernel — by
 * construction the slice of the global bitmap.  Staging: |D| * ((n + 31) / 32) * 4 bytes per context (per part: n_p for n), nothing
 * of the size of n crosses PCIe; an allocation that fails is returned as IDIST_ERR_HIP, nothing is truncated.
 * Host pointers; blocks until done; ctx / p are the `&mut Search` as in the bitmap calls.
 * Conditions over several attributes and unions of intervals: the attribute tables below.
 * Out of scope: testing the attribute inside the select / scan kernels instead of through bitmaps, device-pointer / stream variants
 * and idist_search_batch_sharded. */
typedef struct idist_attr idist_attr;
idist_status idist_attr_new(const idist_index* idx, const uint32_t* values /* [n], PointId order */, idist_attr** out);
idist_status idist_partitioned_attr_new(const idist_partitioned* p, const uint32_t* values /* [N], global-id order */, idist_attr** out);
void idist_attr_free(idist_attr* a);
idist_status idist_search_batch_attr(const idist_index* idx, idist_search_ctx* ctx, const idist_attr* attr, const float* queries, uint32_t nq,
                                     const uint32_t* lo, const uint32_t* hi, uint32_t n_cond, /* 1 or nq */
                                     uint32_t k, int32_t max_rungs,
                                     uint32_t* out_pid, float* out_dist,      /* nq*k */
                                     uint32_t* out_count, uint32_t* out_rung, /* nq; out_rung may be NULL */
                                     uint32_t* out_counters);                 /* nq*3 or NULL */
idist_status idist_search_batch_range_attr(const idist_index* idx, idist_search_ctx* ctx, const idist_attr* attr, const float* queries,
                                           uint32_t nq, const float* radius, uint32_t n_radius,
                                           const uint32_t* lo, const uint32_t* hi, uint32_t n_cond, /* 1 or nq */
                                           int32_t max_rungs, uint64_t max_total,
                                           uint64_t* out_lims, uint32_t* out_rung, uint32_t* out_counters);
idist_status idist_partitioned_search_batch_attr(idist_partitioned* p, const idist_attr* attr, const float* queries, uint32_t nq,
                                                 const uint32_t* lo, const uint32_t* hi, uint32_t n_cond, /* 1 or nq */
                                                 uint32_t k, int32_t max_rungs,
                                                 uint32_t* out_pid, float* out_dist,      /* nq*k, global ids */
                                                 uint32_t* out_count,                     /* nq */
                                                 uint32_t* out_rung,                      /* [nq][n_parts] or NULL */
                                                 uint32_t* out_counters);                 /* nq*3 or NULL */
idist_status idist_partitioned_search_batch_range_attr(idist_partitioned* p, const idist_attr* attr, const float* queries, uint32_t nq,
                                                       const float* radius, uint32_t n_radius,
                                                       const uint32_t* lo, const uint32_t* hi, uint32_t n_cond, /* 1 or nq */
                                                       int32_t max_rungs, uint64_t max_total,
                                                       uint64_t* out_lims,        /* nq + 1 */
                                                       uint32_t* out_rung,        /* [nq][n_parts] or NULL */
                                                       uint32_t* out_counters);   /* nq*3 or NULL */
/* HIP-event duration (ms) of the bitmap kernel of the last idist_search_batch_attr / idist_search_batch_range_attr through ctx;
 * 0 before the first one, when that call had nothing to find, and with IDIST_KERNEL_EVENTS=0.  After a partitioned attribute call
 * idist_partitioned_last_allowed_slice_ms reports the parts' bitmap kernels, summed, instead of uploads plus slices. */
idist_status idist_search_ctx_attr_bitmap_ms(idist_search_ctx* ctx, float* ms);
/* The bitmap kernel on its own (the role idist_allowed_slice_device plays for the slice): d_values [n], d_lo / d_hi [n_sets], d_out
 * [n_sets][(n + 31) / 32], all u32 in the memory of `device`.  Bit i of out[s] = d_lo[s] <= d_values[i] && d_values[i] <= d_hi[s],
 * unsigned, for i < n; the bits at positions >= n of a row's last word are written as 0.  Every output word is written exactly once
 * (no atomics, nothing to clear first, the same bytes whatever the grid); nothing is read past d_values[n - 1], nothing is written
 * past a row's last word.  n == 0 or n_sets == 0: nothing is done.  Enqueued on `hip_stream` (a hipStream_t, may be NULL) without
 * synchronising. */
idist_status idist_attr_bitmaps_device(const void* d_values, uint32_t n, const void* d_lo, const void* d_hi, uint32_t n_sets,
                                       void* d_out, int32_t device, void* hip_stream);

/* ---- attribute tables: several u32 columns per point, AND / OR conditions per query ------------------------- */
/* Real filters are "tenant = 7 AND day in [100, 200]" or "category in {3, 17, 42}": several attributes, unions of intervals.  An
 * idist_attr is a TABLE of n_cols columns (1 to 64; anything else is IDIST_ERR_INVALID_ARG); idist_attr_new is its n_cols == 1 case.
 *   values      [n_cols][n] u32, column after column, column 0 first: column c is values + c * n, in PointId order (partitioned:
 *               [n_cols][N], global-id order; every non-empty part holds [n_cols][n_p], its slice of every column, on its own device).
 *               n == 0 stays legal (values may be NULL).  Binding, immutability, sharing and idist_attr_free: as above.
 *   the interval calls above accept a table and test COLUMN 0; given a one-column attribute they launch exactly what they launched.
 *   a clause    {col, lo, hi}: lo <= values[col][i] && values[col][i] <= hi, UNSIGNED (lo > hi: the empty clause).
 *   a condition an OR of conjunctions, a conjunction an AND of clauses (DNF): conjunction j = the clauses [and_lims[j], and_lims[j + 1])
 *               — none: TRUE; condition c = the conjunctions [or_lims[c], or_lims[c + 1]) — none: FALSE.  The same column may appear
 *               more than once in a conjunction (an intersection), conjunctions may overlap, "not equal to x" is the two conjunctions
 *               [0, x - 1] and [x + 1, 0xFFFFFFFF]: there is no NOT.  No cap on clauses or conjunctions beyond the u32 limits.
 *   n_cond      1: one condition for the whole batch; nq: one per query — as n_radius.  nq == 0 is no error.
 * IDIST_ERR_INVALID_ARG: n_cond neither 1 nor nq; a null conds, and_lims or or_lims (clauses may be NULL when there is none);
 * and_lims[0] or or_lims[0] not 0; a lims array that decreases (the message names the entry); a clause whose col >= n_cols (the
 * message names the condition and the clause).
 * DEFINITION: let bits[c] be the bitmap of condition c (bit i = the condition evaluated on point i, the bits at positions >= n
 * zero).  Every output of a call below equals, bit for bit, the output of the bitmap call it is listed with given
 * (bits, n_cond, set_of = NULL) — with n_cond == 1: one set and set_of all zero:
 *   idist_search_batch_match                     idist_search_batch_allowed_sets
 *   idist_search_batch_range_match               idist_search_batch_range_allowed_sets       (results: idist_search_ctx_range_fetch)
 *   idist_partitioned_search_batch_match         idist_partitioned_search_batch_allowed_sets, bitmaps over the global ids
 *   idist_partitioned_search_batch_range_match   idist_partitioned_search_batch_range_allowed_sets  (idist_partitioned_range_fetch)
 * and everything else comes from those calls, as for the interval calls, which are the special case of one conjunction of one
 * clause {0, lo, hi}.
 * The conditions are grouped on the host: conditions that are equal as encoded — and those that differ only in the order of the
 * clauses within a conjunction — share one bitmap, D being the distinct ones; set_of and D as one flat program are uploaded; one
 * kernel on the context's stream evaluates the program over the columns into the |D| bitmaps where the restricted search reads
 * them (idist_search_ctx_attr_bitmap_ms; the parts, summed: idist_partitioned_last_allowed_slice_ms), every part over its own
 * slice on its own stream.  Staging: |D| * ((n + 31) / 32) * 4 bytes per context, never nq bitmaps when the conditions repeat; an
 * allocation that fails is IDIST_ERR_HIP, nothing is truncated.  Host pointers; blocks until done.
 * Out of scope: NOT, testing the attributes inside the select / scan kernels, device-pointer / stream variants and
 * idist_search_batch_sharded. */
typedef struct idist_attr_clause { uint32_t col, lo, hi; } idist_attr_clause;   /* lo <= v[col][i] && v[col][i] <= hi, UNSIGNED */
typedef struct idist_attr_conds {
    const idist_attr_clause* clauses; /* [and_lims[n_and]]; may be NULL when there is none */
    const uint32_t* and_lims;         /* [n_and + 1], and_lims[0] = 0, non-decreasing: conjunction j = AND of clauses [and_lims[j], and_lims[j + 1]); none: TRUE */
    const uint32_t* or_lims;          /* [n_cond + 1], or_lims[0] = 0, non-decreasing; n_and = or_lims[n_cond]: condition c = OR of conjunctions [or_lims[c], or_lims[c + 1]); none: FALSE */
    uint32_t n_cond;                  /* 1: one condition for the batch; nq: one per query (as n_radius) */
} idist_attr_conds;
/* values [n_cols][n]: column c is values + c * n, PointId order (partitioned: [n_cols][N], global-id order) */
idist_status idist_attr_new_columns(const idist_index* idx, const uint32_t* values, uint32_t n_cols, idist_attr** out);
idist_status idist_partitioned_attr_new_columns(const idist_partitioned* p, const uint32_t* values, uint32_t n_cols, idist_attr** out);
idist_status idist_search_batch_match(const idist_index* idx, idist_search_ctx* ctx, const idist_attr* attr, const float* queries, uint32_t nq,
                                      const idist_attr_conds* conds, uint32_t k, int32_t max_rungs,
                                      uint32_t* out_pid, float* out_dist,      /* nq*k */
                                      uint32_t* out_count, uint32_t* out_rung, /* nq; out_rung may be NULL */
                                      uint32_t* out_counters);                 /* nq*3 or NULL */
idist_status idist_search_batch_range_match(const idist_index* idx, idist_search_ctx* ctx, const idist_attr* attr, const float* queries,
                                            uint32_t nq, const float* radius, uint32_t n_radius, const idist_attr_conds* conds,
                                            int32_t max_rungs, uint64_t max_total,
                                            uint64_t* out_lims, uint32_t* out_rung, uint32_t* out_counters);
idist_status idist_partitioned_search_batch_match(idist_partitioned* p, const idist_attr* attr, const float* queries, uint32_t nq,
                                                  const idist_attr_conds* conds, uint32_t k, int32_t max_rungs,
                                                  uint32_t* out_pid, float* out_dist,      /* nq*k, global ids */
                                                  uint32_t* out_count,                     /* nq */
                                                  uint32_t* out_rung,                      /* [nq][n_parts] or NULL */
                                                  uint32_t* out_counters);                 /* nq*3 or NULL */
idist_status idist_partitioned_search_batch_range_match(idist_partitioned* p, const idist_attr* attr, const float* queries, uint32_t nq,
                                                        const float* radius, uint32_t n_radius, const idist_attr_conds* conds,
                                                        int32_t max_rungs, uint64_t max_total,
                                                        uint64_t* out_lims,        /* nq + 1 */
                                                        uint32_t* out_rung,        /* [nq][n_parts] or NULL */
                                                        uint32_t* out_counters);   /* nq*3 or NULL */
/* The kernel on its own: d_values [n_cols][col_pitch] (col_pitch >= n: elements between columns), the program of n_sets conditions in
 * device memory (d_clauses [.][3] u32 as idist_attr_clause, d_and_lims, d_or_lims [n_sets + 1]; d_clauses may be NULL for a program
 * without clauses), d_out [n_sets][(n + 31) / 32].  The contract of idist_attr_bitmaps_device: every output word written exactly
 * once, the same bytes whatever the grid, the bits at positions >= n zero, no column read past its element n - 1, nothing written
 * past a row's last word; n == 0 or n_sets == 0: nothing is done.  The program is the caller's: its limits are not checked, and a
 * clause whose col >= n_cols matches nothing.  Enqueued on hip_stream without synchronising, as idist_attr_bitmaps_device. */
idist_status idist_attr_match_bitmaps_device(const void* d_values, uint32_t n, uint32_t n_cols, uint64_t col_pitch,
                                             const void* d_clauses, const void* d_and_lims, const void* d_or_lims, uint32_t n_sets,
                                             void* d_out, int32_t device, void* hip_stream);

/* ---- grouped search: the nearest point of each of the k nearest groups --------------------------------------- */
/* Rows are often chunks of documents, frames of videos, offers of one product: the caller wants the k nearest DOCUMENTS, each
 * represented by its nearest chunk ("collapse" / "group_by").  The group of a point is one column of an attribute table:
 *   attr        a table bound to idx (as for idist_search_batch_match); group_col < n_cols, anything else is IDIST_ERR_INVALID_ARG
 *               and the message names the column count.  g(i) = values[group_col][i].  All 2^32 values are legal groups, 0 and
 *               0xFFFFFFFF included.
 *   conds       NULL: no restriction, A is every point.  Otherwise exactly the argument of idist_search_batch_match: the same
 *               checks, the same grouping into distinct conditions, the same bitmap kernel; A is the query's own set.
 *   k, max_rungs, null pointers: the error cases of idist_search_batch_allowed_sets (1 <= k <= ef_search).  nq == 0 is no error.
 * DEFINITION.  The ladder is E[0] = ef_search, E[r + 1] = min(4 E[r], IDIST_MAX_EF).  collapse(L) of a list L ordered by (raw distance
 * bits, id): walk L in order, keep an entry iff it is in A and no earlier KEPT entry has its group, stop after k kept entries.  For
 * one query:
 *   1. n == 0, ef_search == 0 or |A| == 0: count 0, rung IDIST_RUNG_NONE.
 *   2. the start rule of idist_search_batch_allowed_sets, unchanged: |A| <= k goes to the exact step; otherwise r0 is the first
 *      permitted r with E[r] |A| >= k n (64-bit integers); none: the exact step.
 *   3. for r = r0, r0 + 1, ... among the permitted rungs: L = the result of Hnsw::search at ef_search = E[r], raw distances; if
 *      collapse(L) has k entries it is the answer, the rung is r, the query stops.
 *   4. exact: T = all of A ordered by (raw canonical distance bits, id); the answer is collapse(T), the rung IDIST_RUNG_EXACT, the
 *      count min(k, number of distinct groups in A).
 *   5. distances go through the metric's report once, at the end, on the [nq][k] result.  Padding: IDIST_INVALID / +inf, 0 in
 *      out_group.  out_group[q][i] is the group of result i.  out_counters sums {n_dist, n_exp0, n_expU} over the rungs the query
 *      ran; the exact step adds nothing.
 * As in the several-sets call: a later rung that does not fit a wave's LDS ends the ladder (rung 0: the failure is returned); strict
 * ties are retried inside; every row is what the call returns for that query alone; host pointers, the call blocks until done;
 * ctx is the `&mut Search`, idx is never mutated.
 * Two consequences the tests rest on:
 *   - every result row has pairwise distinct groups, and with max_rungs == 0 it is the TRUE answer: the k groups whose nearest
 *     allowed member is nearest, each represented by that member;
 *   - IDENTITY: when every point is its own group (g(i) = i), every output — ids, order, distances, count, rung, counters — equals
 *     that of idist_search_batch_match with the same conds, bit for bit; with conds == NULL that of idist_search_batch_allowed with
 *     every bit set.
 * The rungs launch the search kernels of the several-sets call; one kernel collapses a rung's lists (a set of seen groups in LDS,
 * sized by k); the exact step runs in rounds of the restricted search's scan over A minus the groups found so far, at most k of
 * them (idist_search_ctx_allowed_kernel_ms: the collapse under select_ms, the rounds under exact_ms).  An unrestricted call
 * uploads no bitmap.
 * Out of scope: more than one member per group, the partitioned index, device-pointer / stream variants,
 * idist_search_batch_sharded. */
idist_status idist_search_batch_grouped(const idist_index* idx, idist_search_ctx* ctx, const idist_attr* attr, uint32_t group_col,
                                        const float* queries, uint32_t nq,
                                        const idist_attr_conds* conds,           /* NULL: no restriction */
                                        uint32_t k, int32_t max_rungs,
                                        uint32_t* out_pid, float* out_dist,      /* nq*k */
                                        uint32_t* out_group,                     /* nq*k or NULL */
                                        uint32_t* out_count, uint32_t* out_rung, /* nq; out_rung may be NULL */
                                        uint32_t* out_counters);                 /* nq*3 or NULL */
/* The collapse kernel on its own (the role idist_attr_bitmaps_device plays for the bitmap kernel): d_pid / d_dist [nq][width] (u32 ids,
 * f32 bit patterns), d_count [nq], d_groups [n] u32, d_bits [nq][(n + 31) / 32] or NULL (everything allowed), all in the memory of
 * `device`; 1 <= k <= IDIST_MAX_EF.  Row q of d_out_pid / d_out_dist / d_out_group [nq][k] is collapse of the first min(count,
 * width) entries of list q with A = the bits of row q of d_bits, padded as above; d_out_count[q] is the number kept.  Every output
 * word is written exactly once; nothing beyond a list's count is read; ids >= n are never dereferenced and count as not allowed.
 * nq == 0: nothing is done.  Enqueued on `hip_stream` (a hipStream_t, may be NULL) without synchronising. */
idist_status idist_grouped_collapse_device(const void* d_pid, const void* d_dist, const void* d_count, uint32_t nq, uint32_t width,
                                           const void* d_groups /* u32 [n] */, uint32_t n,
                                           const void* d_bits /* [nq][(n+31)/32] or NULL: everything allowed */,
                                           uint32_t k, void* d_out_pid, void* d_out_dist, void* d_out_group, void* d_out_count,
                                           int32_t device, void* hip_stream);

/* Point::distance for id lists (core/lib.rs:780-782 as used at :709-710): out[q][i] =
 * distance(queries[q], points[ids[q][i]]) for i < n_ids; IDIST_INVALID ids give +inf.
 * Host pointers. The batched gather-L2 kernel on its own. */
idist_status idist_distance_batch(const idist_index* idx, const float* queries, uint32_t nq,
                                  const uint32_t* ids, uint32_t n_ids, float* out_dist);

/* The walk's reject filter for id lists, on its own: out[q][i] = a LOWER BOUND of
 * distance(queries[q], points[ids[q][i]]) in the index's metric, computed from the one-byte-per-coordinate copy of the row
 * alone with the walk's own loads and arithmetic — `Search::push` (core/lib.rs:704-720) is spared the f32 row of a candidate
 * whose bound exceeds the furthest distance of a full `nearest`.  0 where there is no bound (IDIST_INVALID ids, rows with a
 * non-finite coordinate, indexes without the copy).  Host pointers.  tests/ hold the bound against idist_distance_batch;
 * bench.py uses one pass over all rows as the known byte count its traffic counters are calibrated on. */
idist_status idist_filter_bound_batch(const idist_index* idx, const float* queries, uint32_t nq,
                                      const uint32_t* ids, uint32_t n_ids, float* out_bound);

/* Exact k nearest neighbours by exhaustive scan with the canonical distance (the
 * brute-force check of tests/all.rs:60-67); host pointers. */
idist_status idist_bruteforce(const idist_index* idx, const float* queries, uint32_t nq,
                              uint32_t k, uint32_t* out_pid, float* out_dist);

/* The normalisation of IDIST_METRIC_COSINE on its own: out_rows[i] = x^ of rows[i] (n x dim, row-major; may be `rows` itself),
 * out_norm2[i] (may be NULL) = s(rows[i]), the canonical L2SQ distance of the row to the origin.  Host pointers.  What a caller
 * needs to reproduce a cosine index with an L2SQ one, bit for bit. */
idist_status idist_normalize_batch(const float* rows, uint32_t n, uint32_t dim, float* out_rows, float* out_norm2,
                                   int32_t device);

/* The augmentation of IDIST_METRIC_DOT on its own (steps 1-4 of its definition).  rows: n x dim, row-major.  bound_in: 0 = derive S
 * from the rows, else the S to use (finite, > 0, >= every finite s(x): IDIST_ERR_INVALID_ARG otherwise, naming a row).
 * out_rows (n x (dim + 1), may be NULL when only the norms and the bound are wanted) = x~; out_norm2 (n, may be NULL) = s(x);
 * out_bound (may be NULL) = S.  Queries are augmented by appending a 0.  Host pointers; `rows` is only read.  What a caller needs
 * to reproduce a DOT index with an L2SQ one bit for bit, and to find the common bound of the parts of a partitioned index. */
idist_status idist_dot_augment_batch(const float* rows, uint32_t n, uint32_t dim, float bound_in, float* out_rows,
                                     float* out_norm2, float* out_bound, int32_t device);

#ifdef __cplusplus
}
#endif
#endif /* IDIST_H */
