/*
 * pandrs_hip.h — C ABI of libpandrs_hip.so, the MI355X (gfx950) groupby-aggregate /
 * hash-join engine that sits behind PandRS's GroupBy / agg() / join API.
 *
 * The reference (cool-japan/pandrs) exposes NO FFI for this path: the
 * seams a maintainer would bind are Rust methods.  Every entry point below names the
 * reference interface it replaces (file:line into the reference tree).
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types.
 *   - every function returns a pandrs_hip_status (0 = ok); on failure a thread-local
 *     message is available from pandrs_hip_last_error().  Nothing panics/aborts
 *     across the ABI (reference: Result<T, pandrs::Error>, src/core/error.rs:6): every
 *     entry point catches C++ exceptions of its host code (std::bad_alloc ->
 *     PANDRS_HIP_ERR_OUT_OF_MEMORY, anything else -> PANDRS_HIP_ERR_COMPUTATION).
 *   - `mem_space` says where the caller's column / output pointers live:
 *     PANDRS_HIP_MEM_HOST (library stages H2D/D2H itself) or PANDRS_HIP_MEM_DEVICE
 *     (pointers are HBM addresses on the context's device; nothing crosses PCIe).
 *     Any other value of a `mem_space` / `out_mem_space` argument is
 *     PANDRS_HIP_ERR_INVALID_ARGUMENT at every entry point, before anything is read.
 *     Device inputs must be COMPLETE when a call starts: the context's stream is
 *     non-blocking, so a caller that produced them on another stream synchronises that
 *     stream first.  Device outputs are complete when the call returns.
 *   - caller pointers are never retained past return (reference columns are Arc<[T]>
 *     borrowed for the call, src/column/int64_column.rs:52-56).
 *   - a context owns one HIP stream and a workspace arena; calls on ONE context are
 *     serialised by an internal mutex, distinct contexts run concurrently
 *     (reference re-entrancy requirement: tests/concurrency_test.rs:351-398).
 *   - null masks are LSB-first bitmaps, bit = 1 => null (src/core/column.rs:163-177),
 *     may be NULL (= no nulls).
 */
#ifndef PANDRS_HIP_H
#define PANDRS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PANDRS_HIP_ABI_VERSION 1

/* status codes; the names map onto pandrs::Error variants (src/core/error.rs) */
typedef enum pandrs_hip_status {
    PANDRS_HIP_OK = 0,
    PANDRS_HIP_ERR_INVALID_ARGUMENT = 1,   /* Error::InvalidInput / ColumnNotFound at the shim */
    PANDRS_HIP_ERR_TYPE_MISMATCH = 2,      /* Error::ColumnTypeMismatch (join.rs:98-104) */
    PANDRS_HIP_ERR_OPERATION_FAILED = 3,   /* Error::OperationFailed (aggregation.rs:744-752, lazy.rs:377-382) */
    PANDRS_HIP_ERR_COMPUTATION = 4,        /* Error::Computation(String) — device failures (src/gpu/mod.rs:206-210) */
    PANDRS_HIP_ERR_OUT_OF_MEMORY = 5,
    PANDRS_HIP_ERR_NOT_INITIALIZED = 6,
    PANDRS_HIP_ERR_BELOW_THRESHOLD = 7     /* fewer rows than GpuConfig.min_size_threshold: the caller keeps its CPU path
                                              (src/optimized/split_dataframe/gpu.rs:30-32); nothing was computed */
} pandrs_hip_status;

/* column element types.  Layouts are the reference's own:
 *   I64      Int64Column.data   Arc<[i64]>  (src/column/int64_column.rs:52-56)
 *   F64      Float64Column.data Arc<[f64]>  (src/column/float64_column.rs:9-13)
 *   U32CODE  StringColumn.indices Arc<[u32]> — global string-pool codes, equal string
 *            <=> equal code (src/column/string_column.rs:26-32, string_pool.rs:28-53)
 *   BOOLBITS BooleanColumn.data BitMask, LSB-first packed (src/column/boolean_column.rs:10-15)
 *   CELL64   (no reference counterpart; KEY columns only) already-normalised 8-byte key cells — the form
 *            group keys are returned in and pandrs_hip_shuffle_fetch delivers: i64 value / canonical
 *            f64 bits / zero-extended code / bool bit.  Equal cells <=> equal keys. */
typedef enum pandrs_hip_dtype {
    PANDRS_HIP_I64 = 0,
    PANDRS_HIP_F64 = 1,
    PANDRS_HIP_U32CODE = 2,
    PANDRS_HIP_BOOLBITS = 3,
    PANDRS_HIP_CELL64 = 4
} pandrs_hip_dtype;

/* AggregateOp, same order as src/optimized/split_dataframe/group/types.rs:11-34 */
typedef enum pandrs_hip_agg_op {
    PANDRS_HIP_AGG_SUM = 0,
    PANDRS_HIP_AGG_MEAN = 1,
    PANDRS_HIP_AGG_MIN = 2,
    PANDRS_HIP_AGG_MAX = 3,
    PANDRS_HIP_AGG_COUNT = 4,
    PANDRS_HIP_AGG_STD = 5,
    PANDRS_HIP_AGG_VAR = 6,
    PANDRS_HIP_AGG_MEDIAN = 7,
    PANDRS_HIP_AGG_FIRST = 8,
    PANDRS_HIP_AGG_LAST = 9,
    PANDRS_HIP_AGG_CUSTOM = 10,  /* always PANDRS_HIP_ERR_OPERATION_FAILED (aggregation.rs:744) */
    /* beyond AggregateOp: the legacy frame's AggFunc::Nunique (src/dataframe/groupby.rs:514-519, SURVEY.md
     * 8f item 2) — the number of distinct non-null values of the group (sort + dedup: values equal under
     * `==`, so -0.0 and 0.0 are one value and every NaN is its own), 0.0 for a group without values (:467). */
    PANDRS_HIP_AGG_NUNIQUE = 11
} pandrs_hip_agg_op;

/* JoinType, src/optimized/split_dataframe/join.rs:11-20 */
typedef enum pandrs_hip_join_type {
    PANDRS_HIP_JOIN_INNER = 0,
    PANDRS_HIP_JOIN_LEFT = 1,
    PANDRS_HIP_JOIN_RIGHT = 2,
    PANDRS_HIP_JOIN_OUTER = 3
} pandrs_hip_join_type;

typedef enum pandrs_hip_mem_space {
    PANDRS_HIP_MEM_HOST = 0,
    PANDRS_HIP_MEM_DEVICE = 1
} pandrs_hip_mem_space;

/* Mirrors GpuConfig (src/gpu/mod.rs:18-44). */
typedef struct pandrs_hip_config {
    int32_t enabled;             /* GpuConfig.enabled */
    int32_t device_id;           /* GpuConfig.device_id */
    int64_t memory_limit;        /* GpuConfig.memory_limit, bytes; 0 = no limit */
    int32_t fallback_to_cpu;     /* GpuConfig.fallback_to_cpu — honoured by the CALLER (shim keeps the
                                    reference CPU path); this library never computes on the CPU */
    int32_t use_pinned_memory;   /* GpuConfig.use_pinned_memory: host columns of a MEM_HOST call are page-locked
                                    (hipHostRegister) for the duration of the call, so their H2D copies are DMA */
    int64_t min_size_threshold;  /* GpuConfig.min_size_threshold (src/gpu/mod.rs:41).  Honoured once a config has been
                                    passed to pandrs_hip_init: the frame-level entry points (groupby_agg, groupby_indices,
                                    join_indices, join_groupby_sum, reduce_*) return PANDRS_HIP_ERR_BELOW_THRESHOLD for
                                    fewer rows.  Without an explicit config the threshold is 0: this library has no CPU
                                    path of its own to prefer. */
} pandrs_hip_config;

/* One typed column view.  `data` element type per `dtype`; `null_mask` may be NULL. */
typedef struct pandrs_hip_column {
    const void *data;
    const uint8_t *null_mask;
    int32_t dtype;      /* pandrs_hip_dtype */
    int32_t reserved;
} pandrs_hip_column;

/* One requested aggregate: (index into vals[], op).  Replaces the
 * (String column, AggregateOp, String alias) triples of GroupBy::aggregate
 * (aggregation.rs:763-767); alias naming stays on the host side. */
typedef struct pandrs_hip_agg_spec {
    int32_t col;
    int32_t op;         /* pandrs_hip_agg_op */
} pandrs_hip_agg_spec;

/* Per-call measurements, for the bench (SURVEY.md §8b "pandrs_hip_get_timings"). */
#define PANDRS_HIP_MAX_PHASES 12
typedef struct pandrs_hip_timings {
    double total_ms;                          /* hipEvent time, whole call on the ctx stream */
    double phase_ms[PANDRS_HIP_MAX_PHASES];   /* per phase, see PANDRS_HIP_PHASE_*: from the phase's first launch to its last (phases
                                                 of one call may overlap); small calls (the two-launch path) record none */
    int64_t algorithmic_bytes;                /* SURVEY.md §8d formula for this call */
    int64_t n_partitions;                     /* radix fan-out chosen (0: the small-call path; -1: hot-key absorb pass with a COMPACT spill —
                                                 the rest of the rows went through a run of their own; -2: rows clustered by key, one pass
                                                 over the original columns and no partition at all; fused join: the probe side's fan-out,
                                                 0 = general fallback) */
    int64_t table_slots;                      /* LDS hash-table slots per partition */
    int64_t retries;                          /* overflow retries taken; 100 + retries: full LDS tables handed their unplaced rows to a
                                                 run of their own instead (groupby; the estimate was too low).  (fused join: 1 = the partitioned pair output overflowed a
                                                 region and the one-cursor emission answered; 2 = the groupby engine refused the
                                                 pre-partitioned pairs — a full LDS table — and the whole call was repeated with
                                                 the one-cursor emission) */
    int64_t estimated_groups;
    int64_t absorbed_rows;                    /* rows folded by the hot-key absorb pass in front of the radix path (0: it did not run) */
} pandrs_hip_timings;

enum {
    PANDRS_HIP_PHASE_STAGE_IN = 0,    /* H2D staging (host mem_space only) */
    PANDRS_HIP_PHASE_ESTIMATE = 1,    /* sampled cardinality estimate */
    PANDRS_HIP_PHASE_HISTOGRAM = 2,   /* radix histogram */
    PANDRS_HIP_PHASE_SCAN = 3,        /* exclusive scan of bucket counts */
    PANDRS_HIP_PHASE_SCATTER = 4,     /* LDS-staged radix scatter */
    PANDRS_HIP_PHASE_AGGREGATE = 5,   /* per-partition LDS hash aggregate + compaction */
    PANDRS_HIP_PHASE_BUILD = 6,       /* join: build side */
    PANDRS_HIP_PHASE_PROBE = 7,       /* join: probe count + write */
    PANDRS_HIP_PHASE_GATHER = 8,
    PANDRS_HIP_PHASE_OTHER = 9,
    PANDRS_HIP_PHASE_PREPARTITION = 10  /* first pass (64 buckets) of a two-pass radix partition: fan-outs >= 6144 */
};

typedef struct pandrs_hip_ctx pandrs_hip_ctx;

/* ---- library lifetime ----------------------------------------------------------------
 * Replaces init_gpu / get_gpu_manager (src/gpu/mod.rs:214-282).  Idempotent. */
int32_t pandrs_hip_abi_version(void);
int32_t pandrs_hip_init(const pandrs_hip_config *cfg /* NULL = defaults */);
int32_t pandrs_hip_shutdown(void);
int32_t pandrs_hip_device_count(int32_t *out_count);
const char *pandrs_hip_last_error(void);

/* ---- contexts (one stream + workspace per context) ------------------------------------ */
int32_t pandrs_hip_ctx_create(int32_t device_id, pandrs_hip_ctx **out_ctx);
int32_t pandrs_hip_ctx_destroy(pandrs_hip_ctx *ctx);
int32_t pandrs_hip_ctx_synchronize(pandrs_hip_ctx *ctx);
/* Pre-size the workspace arena (bytes) so the first timed call does not pay hipMalloc. */
int32_t pandrs_hip_ctx_reserve(pandrs_hip_ctx *ctx, int64_t workspace_bytes);
/* Number of device allocations (hipMalloc) the library has made in this process: workspace arenas grow but never
 * shrink, so a repeated call of the same shape adds none — tests assert that on the steady state. */
int32_t pandrs_hip_alloc_events(int64_t *out_device_allocations);
/* Bytes of workspace filled by the "poison_workspace" testing knob (below) since the library was loaded; stays where it
 * is while the knob is 0. */
int32_t pandrs_hip_workspace_poisoned_bytes(int64_t *out_bytes);
/* Tuning / testing knobs — EVERY name the library accepts (all default to 0 = automatic unless noted; the tests and
 * experiments/ use them to force individual code paths; tests/test_abi.py checks this list against capi.hip):
 *  planning
 *   "groups_hint"       expected number of groups (skips the sampled estimate)
 *   "partitions"        force the radix fan-out P
 *   "p_max"             lower the fan-out cap (forces the two-level path above it)
 *   "p_target"          rounds heuristic: take several aggregate rounds only above this fan-out (default: 8192 where the lean kernel answers, else 3072)
 *   "src_per_round"     force the number of value columns folded per aggregate round
 *   "load_pct"          LDS table load factor in percent (default 70)
 *  partition (scatter) pass
 *   "scatter_staged"    1 (default) = stage columns through LDS and write contiguous per-partition runs; 0 = direct stores
 *   "scatter_threads"   1024 (default) or 512 threads per scatter workgroup
 *   "shared_cursors"    1 (default) = one write cursor per (partition, XCD group); 0 = private cursors per workgroup
 *   "exact_partition"   1 = always the exact histogram + scan layout, never the sampled-capacity layout
 *  aggregate pass
 *   "agg_v1"            1 = never the lean persistent aggregate (aggregate2.hip); the round-1 kernel answers
 *   "generic_aggregate" 1 = the descriptor-driven generic instantiation of the round-1 kernel
 *   "agg_depth"         register-ring depth of the lean aggregate (2..4; default 3)
 *   "agg_ablate"        experiments only: switch parts of the lean aggregate off (see experiments/agg2_ablate.py)
 *   "sort_digit_bits"   experiments only: widest radix digit of pandrs_hip_sort_indices, 4 ... 8 (0 = the default, 8;
 *                       experiments/sort_bench.py --digit-bits)
 *   "topk_path"         tests / experiments: 1 = pandrs_hip_topk always sorts the whole column, -1 = it always selects; 0 = the
 *                       default, by topk_cutover (experiments/topk_bench.py)
 *   "isin_path"         tests / experiments: 1 = pandrs_hip_isin takes the LDS set wherever the list fits, 2 = it always builds the
 *                       global set; 0 = the default, by the list's size (isin_lds_max_values; experiments/predicate_bench.py)
 *   "predicate_path"    tests / experiments: 1 = pandrs_hip_predicate converts every I64 cell with (double)v in its loop; 0 = the
 *                       default, integers compared against the interval the host bisects (the same bits; experiments/predicate_bench.py)
 *   "bin_path"          tests / experiments: 1 = pandrs_hip_bin always takes the search, 2 = it takes the guess wherever the edges
 *                       are evenly spaced; 0 = the default, the guess from bin_guess_min_bins evenly spaced bins on (the same
 *                       codes; experiments/bin_bench.py)
 *   "distinct_path"     tests / experiments: 1 = pandrs_hip_distinct takes the direct (LDS table) path wherever the column's numbers fit
 *                       it, 2 = it always takes the groupby engine; 0 = the default, direct wherever it fits (the same list;
 *                       experiments/distinct_bench.py)
 *   "pivot_path"        tests / experiments: 1 = pandrs_hip_pivot takes the direct (LDS table) path wherever the two key columns fit it,
 *                       2 = it always takes the general path (the groupby engine); 0 = the default, direct wherever it fits (the
 *                       same result; experiments/pivot_bench.py)
 *   "window_quantile_path"  tests / experiments: 1 = pandrs_hip_window_quantile takes the direct (LDS) path, which serves rolling
 *                       windows of at most 44 rows (a wider or expanding window: PANDRS_HIP_ERR_INVALID_ARGUMENT), 2 = it always
 *                       takes the general (wavelet matrix) path; 0 = the default, by the window (experiments/window_quantile_bench.py)
 *   "no_runs"           1 = never the clustered-rows (RUNS) instantiation
 *   "no_direct"         1 = never the few-groups direct path (-1 = allow it below 4 M rows too)
 *   "test_throw"        tests of the exception firewall (ctx may be NULL): 1 = the entry point's host code throws std::bad_alloc
 *                       (-> PANDRS_HIP_ERR_OUT_OF_MEMORY), 2 = std::out_of_range, 3 = a non-std exception, 4 = an oversized
 *                       std::vector::resize (2 - 4 -> PANDRS_HIP_ERR_COMPUTATION, or OUT_OF_MEMORY for bad_alloc); never a crash.
 *                       5 (needs a ctx) = arms the context once: the next engine run that is nested inside a call (a merge of partial
 *                       records, a run over spilled rows) throws std::bad_alloc; that call fails with OUT_OF_MEMORY and the context
 *                       serves the next call as if nothing had happened
 *   "poison_workspace"  tests of the workspace's write-before-read discipline (process-wide; ctx may be NULL): every workspace block the
 *                       library hands itself (each arena whenever a call sizes it, grown or reused, and the one-off tables) is filled
 *                       with the byte (value & 0xFF) on the call's stream before the call uses it; 256 = the zero byte, 0 (default) = off:
 *                       no fill, no launch, no synchronisation.  Resident columns and caller buffers are never touched.
 *                       pandrs_hip_workspace_poisoned_bytes counts what was filled
 *   "no_census"         1 = the group estimate never takes its second stage (a hash-slice census of a tenth of the rows, run when the
 *                       strided sample shows singletons its repeating keys cannot explain: a long tail behind a broad hot class)
 *   "tail_groups_hint"  tests: the group estimate handed to the tail run of the absorb pass's compact spill (0 = its own sample)
 *   "no_overflow_run"   1 = a full LDS table fails the attempt (the call is retried with 4 x the fan-out) instead of handing the rows it
 *                       could not place to a run of their own, whose groups are appended
 *   "sorted_dictionary" 1 = a column of a composite key that is too wide for its share of the 64-bit cell gets its dictionary codes by
 *                       ordering the rows (any cardinality) instead of listing its distinct cells and a hashed look-up per row
 *   "no_chao"           1 = the sampled group estimate is the uniform-occupancy model alone (no Chao1 term: tests, A/B)
 *   "no_absorb"         1 = never the hot-key absorb-and-spill pass in front of the radix path (-1 = whenever it is possible: tests)
 *   "no_hot_image"      1 = the absorb tables start empty (first come, first served) instead of from the sample's most frequent keys
 *   "no_slice"          1 = never cut oversized partitions into row slices; "slice_rows" forces the slice length
 *   "wide_slices"       1 = the pieces of an oversized partition are as long as the cutting threshold (4 x the average partition) instead of
 *                       average-sized (A/B: a piece is one workgroup's job, long pieces are the aggregate pass's tail)
 *   "slice_over"        experiments: a partition is cut when it holds more than this many average partitions' rows (default 2)
 *   "no_clustered"      1 = never the one-pass path for rows clustered by key (sorted input, input grouped by key); "clustered_chunk"
 *                       rows per chunk there, "clustered_max_runs_pct" runs per 100 rows up to which it is taken (default 13)
 *   "no_profile_rounds" 1 = aggregated columns of mixed kinds / op sets go to the older kernel (default: ordered by profile, the lean kernel
 *                       takes up to 4 columns of one profile per round)
 *   "no_burst_kernel"   1 = partitions whose keys arrive in bursts (short runs, keys local in position) are aggregated row per lane by the
 *                       lean kernel instead of 8 consecutive rows per thread
 *   "no_window_bound"   1 = the group estimate never counts distinct keys in windows of consecutive rows (its bound for keys that are
 *                       local in position: nearly sorted input)
 *   "no_lean_rounds"    1 = several aggregate rounds always run the older kernel (default: uniform profiles run the lean kernel once per
 *                       round of <= 4 columns over the same partitions)
 *   "no_table_order"    experiments: 1 = the lean aggregate draws its tables in partition order instead of largest first
 *   "fold_min", "fold_min_multi"  experiments: lanes of a wave in one table slot from which the lean aggregate folds them on the VALU
 *                       (ordinary tables: default 40; pieces of an oversized partition: default 8; 65 = never)
 *   "no_small"          1 = never the two-launch path for calls of <= 2 M rows; "small_chunk" rows per workgroup there
 *   "deterministic"     1 = f64 Sum / Mean / Std / Var re-folded in ascending row order (bit-identical to the
 *                       reference's sequential fold; about 3 x the default time)
 *  join
 *   "join_generic"      1 = always build the join with the general segmented sort
 *   "join_one_pass"     1 = single-pass probe (decoupled look-back) instead of count + emit
 *   "join_no_l2"        1 = fused join->groupby never takes the L2-region path for large build sides
 *   "scatter_wide"      the scatter's wide tile (16 K rows per workgroup, staged in two halves): 1 = whenever its LDS fits, -1 = never;
 *                       default: at fan-outs >= 1024 with two or more 8-byte value columns (>= 1536 with one)
 *   "two_pass"          -1 = the exact radix partition never takes two passes (64-127 buckets, then the rest) at fan-outs >= 6144;
 *                       "two_pass_min_p" = another threshold (tests: also lifts the 4 M-row minimum)
 *   "join_pair_p"       the L2-region probe's minimum pair fan-out (0 = the default)
 *   "join_no_pairpart"  1 = the L2-region probe emits its pairs through one cursor instead of pre-partitioned
 *  Median / Nunique
 *   "median_generic"    1 = always the general segmented-sort pass, never the LDS group-sort path
 * Unknown names are rejected with PANDRS_HIP_ERR_INVALID_ARGUMENT.
 * Diagnostics (environment, read once): PANDRS_HIP_ENGINE_TRACE=1 prints one line per engine attempt (rows, estimate, fan-out, table
 * slots, kernel family, nesting level) on stderr; PANDRS_HIP_DIST_TRACE=1 the wall time of every stage of a distributed groupby. */
int32_t pandrs_hip_ctx_set_option(pandrs_hip_ctx *ctx, const char *name, int64_t value);
int32_t pandrs_hip_get_timings(pandrs_hip_ctx *ctx, pandrs_hip_timings *out);

/* ---- resident columns --------------------------------------------------------------------------
 * The reference's columns are immutable Arc<[T]> buffers (src/column/int64_column.rs:10, float64_column.rs:9,
 * string_column.rs:26) that every operator of the public frame Arc-clones into the split frame
 * (src/optimized/dataframe/transformations.rs:524-577 aggregate, :628-694 join): nothing ever writes to them.  A shim
 * therefore uploads a column ONCE and serves every later aggregate / join on it from HBM:
 *   pandrs_hip_column_upload copies the host column (data + null bitmap, if any) into one device allocation owned by
 *     the context and fills *out_device_col with the device pointers (same dtype); returns after the copy has
 *     completed, so the host buffers may be dropped.  Use the descriptor with PANDRS_HIP_MEM_DEVICE in any entry
 *     point, as often as wanted.
 *   pandrs_hip_column_release frees it (waits for work in flight on the context's stream first); columns still
 *     resident when the context is destroyed are freed with it.  Releasing a descriptor twice, or one that did not
 *     come from column_upload on this context, is PANDRS_HIP_ERR_INVALID_ARGUMENT.
 *   pandrs_hip_resident_bytes reports what the context currently holds (counted against
 *     pandrs_hip_config.memory_limit).
 * The Rust shim keys its handles by the Arc's data pointer and keeps a Weak beside each (integration/rust/
 * hip_shim.rs `ResidentCache`): a dropped column can neither be served stale nor have its address reused while cached. */
int32_t pandrs_hip_column_upload(pandrs_hip_ctx *ctx, const pandrs_hip_column *host_col, int64_t n_rows,
                                 pandrs_hip_column *out_device_col);
int32_t pandrs_hip_column_release(pandrs_hip_ctx *ctx, const pandrs_hip_column *device_col);
int32_t pandrs_hip_resident_bytes(pandrs_hip_ctx *ctx, int64_t *out_bytes, int64_t *out_columns);

/* ---- groupby-aggregate ------------------------------------------------------------------
 * Replaces OptimizedDataFrame::group_by(..)?.aggregate(..)
 *   (src/optimized/split_dataframe/group/grouping.rs:22-115 +
 *    src/optimized/split_dataframe/group/aggregation.rs:500-871)
 * and the inline copy in LazyFrame::execute (src/optimized/lazy.rs:186-404).
 *
 * Semantics (bit-for-bit the reference's fold rules):
 *   - a null key is its own group ("NULL", grouping.rs:74); f64 keys: all NaNs one group,
 *     0.0 != -0.0 (string equality of val.to_string()).
 *   - every aggregate is an f64; I64 Sum wraps in i64 then casts; Mean of nothing = 0.0;
 *     Min/Max whose sentinel is unchanged = 0.0; Count = group size INCLUDING nulls;
 *     Std/Var = two-pass, Bessel; First/Last = value at first/last row, null => 0.0;
 *     Median = middle of the sorted non-null values, even counts average the two middles
 *     (Int64: added in i64 first), no non-null value => 0.0 (aggregation.rs:585-604, :703-722).
 *     Nunique (not an AggregateOp: the legacy frame's AggFunc::Nunique) = number of distinct non-null
 *     values under `==` (-0.0 joins 0.0, every NaN counts), none => 0.0 (src/dataframe/groupby.rs:514-519).
 *   - group order in the output is unspecified (reference: HashMap order).
 *   - value dtypes: I64 / F64 for numeric ops; Count accepts any dtype; anything else =>
 *     PANDRS_HIP_ERR_OPERATION_FAILED (aggregation.rs:748).
 *
 * Two steps so that outputs are caller-allocated after a size query:
 *   1. pandrs_hip_groupby_agg computes on the device and keeps the result in the ctx,
 *      returning n_groups;
 *   2. pandrs_hip_groupby_fetch copies it out and may be called repeatedly until the next
 *      compute call on the same ctx.
 * out_keys[k]     : n_groups 8-byte cells — i64 value / f64 bits / zero-extended u32 code /
 *                   0-1 for bool.  Stringification stays host-side (aggregation.rs:856-860).
 * out_key_null[k] : n_groups bytes, 1 = the NULL group (may be NULL pointer to skip).
 * out_aggs[a]     : n_groups doubles per requested aggregate, in request order.
 */
int32_t pandrs_hip_groupby_agg(pandrs_hip_ctx *ctx, int32_t mem_space,
                               const pandrs_hip_column *keys, int32_t n_keys,
                               int64_t n_rows,
                               const pandrs_hip_column *vals, int32_t n_vals,
                               const pandrs_hip_agg_spec *aggs, int32_t n_aggs,
                               int64_t *out_n_groups);
int32_t pandrs_hip_groupby_fetch(pandrs_hip_ctx *ctx, int32_t mem_space,
                                 uint64_t *const *out_keys, uint8_t *const *out_key_null,
                                 double *const *out_aggs);

/* ---- mergeable partial aggregates (multi-GPU) -----------------------------
 * The reference has no distributed path for groupby (src/distributed is an in-process DataFusion
 * wrapper); these three calls are the pieces of the row-range-sharded plan:
 *   pandrs_hip_groupby_partials : same inputs as groupby_agg, but keeps the un-finalised
 *     per-group states (group size, then per value column: sum, non-null count, min, max as the
 *     requested ops need) so that partials from several row-range shards can be merged.  The
 *     state layout is a pure function of (value dtypes, has-null flags, agg specs): every rank
 *     computes the same layout.  *out_n_state = 8-byte state cells per group (incl. group size).
 *   pandrs_hip_partials_split : buckets the retained partial rows by owner rank
 *     (hash(key) mod n_ranks; the NULL group goes to rank 0) and writes them rank-contiguous as
 *     packed records of W = 2 + n_state 8-byte cells: [key cell, key_null (0/1), states...],
 *     ready for ONE all-to-all; out_counts[r] = records destined to rank r (host array).
 *   pandrs_hip_groupby_merge : consumes concatenated packed records (from all peers), merges
 *     equal keys and finalises the aggregates exactly like groupby_agg; fetch with
 *     pandrs_hip_groupby_fetch.  val_dtypes / val_has_nulls / aggs must equal the producers'. */
int32_t pandrs_hip_groupby_partials(pandrs_hip_ctx *ctx, int32_t mem_space,
                                    const pandrs_hip_column *keys, int32_t n_keys,
                                    int64_t n_rows,
                                    const pandrs_hip_column *vals, int32_t n_vals,
                                    const pandrs_hip_agg_spec *aggs, int32_t n_aggs,
                                    int64_t *out_n_groups, int32_t *out_n_state);
int32_t pandrs_hip_partials_split(pandrs_hip_ctx *ctx, int32_t mem_space, int32_t n_ranks,
                                  uint64_t *out_records /* [n_groups][2 + n_state] */,
                                  int64_t *out_counts /* host, n_ranks */);
int32_t pandrs_hip_groupby_merge(pandrs_hip_ctx *ctx, int32_t mem_space, int32_t key_dtype,
                                 const uint64_t *records /* [n_rows][2 + n_state] */,
                                 int64_t n_rows,
                                 const int32_t *val_dtypes, int32_t n_vals,
                                 const uint8_t *val_has_nulls,
                                 const pandrs_hip_agg_spec *aggs, int32_t n_aggs,
                                 int64_t *out_n_groups);

/* ---- group_by's row -> group assignment ----------------------------------
 * Replaces the body of OptimizedDataFrame::group_by (src/optimized/split_dataframe/group/
 * grouping.rs:22-115), which builds HashMap<Vec<String>, Vec<usize>>: per group, the ascending list
 * of its row indices (:98-103).  GroupBy.groups is a pub field (group/types.rs:52) that filter /
 * transform / aggregate_custom (group/operations.rs:51-435, aggregation.rs:391-497) and
 * par_groupby's sub-frame gathers (grouping.rs:286-328) read.  Device form = CSR:
 * group g has key cells out_keys[k][g] (+ null flags) and rows out_rows[out_offsets[g] ..
 * out_offsets[g+1]), ascending.  Null keys form one group per distinct combination, like the
 * reference's "NULL" strings (grouping.rs:74).  Group order is unspecified (HashMap order there). */
int32_t pandrs_hip_groupby_indices(pandrs_hip_ctx *ctx, int32_t mem_space,
                                   const pandrs_hip_column *keys, int32_t n_keys, int64_t n_rows,
                                   int64_t *out_n_groups);
/* out_keys[k] / out_key_null[k]: n_groups entries each; out_offsets: n_groups + 1; out_rows: n_rows.
 * Any pointer may be NULL to skip that output. */
int32_t pandrs_hip_groupby_indices_fetch(pandrs_hip_ctx *ctx, int32_t mem_space,
                                         uint64_t *const *out_keys, uint8_t *const *out_key_null,
                                         int64_t *out_offsets, int64_t *out_rows);

/* ---- multi-GPU: row shuffle by key owner ("radix all-to-all ... on key") -------------
 * The general exchange for what pre-aggregated partials cannot express (Std/Var/Median, or both
 * sides of a join): every row goes to the rank that owns its key, owner = f(key cell) mod n_ranks,
 * the same function on every rank and for every column that shares the key.  This call buckets ONE
 * shard's rows by owner and keeps them rank-contiguous in the context: key cells, one null byte per
 * row, and every payload column (I64 / F64 as is, U32CODE zero-extended to 8 bytes) with one null
 * byte per row for masked payloads.  out_counts[r] = rows for rank r.  Rows with a NULL key go to
 * the last rank (they form one group, grouping.rs:74) or are dropped when drop_null_keys != 0
 * (they never match in a join, join.rs:112, :152).  After the all-to-all the receiver turns the null
 * bytes into bitmaps (pandrs_hip_bytes_to_bitmap) and calls the ordinary entry points with key
 * dtype PANDRS_HIP_CELL64. */
int32_t pandrs_hip_shuffle_split(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *key,
                                 const pandrs_hip_column *payload, int32_t n_payload, int64_t n_rows,
                                 int32_t n_ranks, int32_t drop_null_keys, int64_t *out_counts,
                                 int64_t *out_n_rows);
/* One 64-bit hash cell per row of a COMPOSITE key (n_keys columns, nulls included): equal key tuples
 * get equal cells on every rank, so the cells can serve as the shuffle key (dtype CELL64) of a
 * multi-key groupby while the key columns themselves travel as payload.  Collisions only co-locate
 * different tuples on one rank; the receiving groupby still separates them. */
int32_t pandrs_hip_key_hash_cells(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *keys,
                                  int32_t n_keys, int64_t n_rows, uint64_t *out_cells);
/* out_cells / out_key_null: out_n_rows entries; out_payload[c] (8 bytes per row) / out_payload_null[c]
 * (1 byte per row; ignored for payloads without a mask).  Any pointer may be NULL to skip it. */
int32_t pandrs_hip_shuffle_fetch(pandrs_hip_ctx *ctx, int32_t mem_space, uint64_t *out_cells,
                                 uint8_t *out_key_null, uint64_t *const *out_payload,
                                 uint8_t *const *out_payload_null);
/* one byte per row (non-zero = set) -> LSB-first bitmap of (n + 7) / 8 bytes (src/core/column.rs:163-177) */
int32_t pandrs_hip_bytes_to_bitmap(pandrs_hip_ctx *ctx, int32_t mem_space, const uint8_t *bytes, int64_t n,
                                   uint8_t *out_bitmap);

/* ---- hash join ------------------------------------------------------------------------------
 * Replaces OptimizedDataFrame::join_impl (src/optimized/split_dataframe/join.rs:76-555) up to
 * the join_indices vector (:146-224); the column gathers (:286-552) are pandrs_hip_gather_*.
 * Order contract = the reference's: left rows ascending; for one left row its matches in
 * ascending right-row order; left/outer misses in place; right/outer unmatched right rows
 * appended ascending.  Null keys never match and null LEFT keys are dropped even for
 * left/outer (join.rs:152).  -1 marks the missing side.  dtype mismatch between the two key
 * columns => PANDRS_HIP_ERR_TYPE_MISMATCH (join.rs:98-104). */
int32_t pandrs_hip_join_indices(pandrs_hip_ctx *ctx, int32_t mem_space,
                                const pandrs_hip_column *left_key, int64_t n_left,
                                const pandrs_hip_column *right_key, int64_t n_right,
                                int32_t how, int64_t *out_n_rows);
int32_t pandrs_hip_join_fetch(pandrs_hip_ctx *ctx, int32_t mem_space,
                              int64_t *out_left_idx, int64_t *out_right_idx);

/* out[i] = idx[i] >= 0 && !null(src, idx[i]) ? src[idx[i]] : fill
 * (join.rs:296-357: misses and nulls become 0 / 0.0 / "" / false, not nulls). */
int32_t pandrs_hip_gather_i64(pandrs_hip_ctx *ctx, int32_t mem_space, const int64_t *src,
                              const uint8_t *src_null_mask, const int64_t *idx, int64_t n,
                              int64_t fill, int64_t *out);
int32_t pandrs_hip_gather_f64(pandrs_hip_ctx *ctx, int32_t mem_space, const double *src,
                              const uint8_t *src_null_mask, const int64_t *idx, int64_t n,
                              double fill, double *out);
int32_t pandrs_hip_gather_u32(pandrs_hip_ctx *ctx, int32_t mem_space, const uint32_t *src,
                              const uint8_t *src_null_mask, const int64_t *idx, int64_t n,
                              uint32_t fill, uint32_t *out);
/* The same gather with the source length in the signature, for either memory space (host columns are
 * staged): src->dtype selects the element — out holds 8 bytes per row for I64 / F64 (fill_bits = the
 * fill value's bit pattern), 4 for U32CODE, and one 0/1 byte per row for BOOLBITS. */
int32_t pandrs_hip_gather_column(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *src,
                                 int64_t n_src, const int64_t *idx, int64_t n, uint64_t fill_bits, void *out);
/* One output column of the join whose pairs this context still holds (the last pandrs_hip_join_indices):
 * out[i] = the gather above with idx = the pairs' left rows (side 0) or right rows (side 1).  This is
 * join_impl's column assembly (join.rs:286-552) with the index pairs never leaving HBM: a shim fetches the
 * joined COLUMNS, not 16 bytes of indices per output row.  `src` lives in src_mem_space (a resident column
 * descriptor from pandrs_hip_column_upload, or a host column, which is staged); `out` (element sizes as for
 * pandrs_hip_gather_column, pandrs_hip_join_indices' *out_n_rows elements) lives in out_mem_space. */
int32_t pandrs_hip_join_gather(pandrs_hip_ctx *ctx, int32_t src_mem_space, const pandrs_hip_column *src,
                               int64_t n_src, int32_t side, uint64_t fill_bits, int32_t out_mem_space, void *out);
/* The join-key column of that frame (join.rs:364-470): the LEFT key's value where the pair has a left row (a null
 * there becomes the fill value), else the RIGHT key's value at the pair's right row (right / outer joins). */
int32_t pandrs_hip_join_gather_key(pandrs_hip_ctx *ctx, int32_t src_mem_space, const pandrs_hip_column *left_key,
                                   int64_t n_left, const pandrs_hip_column *right_key, int64_t n_right,
                                   uint64_t fill_bits, int32_t out_mem_space, void *out);
/* bit-packed source (BooleanColumn), byte-per-row output */
int32_t pandrs_hip_gather_bool(pandrs_hip_ctx *ctx, int32_t mem_space, const uint8_t *src_bits,
                               const uint8_t *src_null_mask, const int64_t *idx, int64_t n,
                               uint8_t fill, uint8_t *out);

/* Fused inner join -> groupby(right payload g).sum(left payload v)  (BASELINE config 5):
 * never materialises the join rows.  Equivalent to inner_join (join.rs:32) followed by
 * group_by(g).aggregate([(v, Sum)]) (aggregation.rs:763).  Fetch with groupby_fetch. */
int32_t pandrs_hip_join_groupby_sum(pandrs_hip_ctx *ctx, int32_t mem_space,
                                    const pandrs_hip_column *left_key,
                                    const pandrs_hip_column *left_val, int64_t n_left,
                                    const pandrs_hip_column *right_key,
                                    const pandrs_hip_column *right_group, int64_t n_right,
                                    int64_t *out_n_groups);

/* ---- sort -------------------------------------------------------------------------------------------------
 * OptimizedDataFrame::sort_by / sort_by_columns (src/optimized/split_dataframe/sort.rs:18-272, exposed on the public
 * frame at src/optimized/dataframe/transformations.rs:1155-1230): out_idx[0 .. n_rows) = the STABLE permutation that
 * orders the rows by keys[0], then keys[1], ... (sort.rs sorts with slice::sort_by, which is stable).
 *   - ascending: n_keys flags (0 = descending), NULL = all ascending.  Descending inverts the comparison; rows that
 *     compare equal on every key keep their original order in both directions.
 *   - nulls sort LAST in both directions ((None, _) => Greater is applied before the direction); two nulls tie and
 *     the comparison moves on to the next key.
 *   - I64: signed order.  F64: numeric order, -0.0 == 0.0 (they tie).  BOOLBITS: false < true.
 *   - U32CODE (string-pool codes) orders by the STRINGS, byte-wise (Rust String: Ord), not by code: code_rank[code]
 *     is the position of the code's string in byte-wise order among the n_codes codes of the (global) pool.  One
 *     table serves every string key.  It lives in mem_space, like the key columns; NULL, 0 when no key is a string.
 *   - CELL64 is not a frame column type: PANDRS_HIP_ERR_INVALID_ARGUMENT.
 *   - documented deviation (NaN): the reference compares NaN as Equal to everything (partial_cmp(..).unwrap_or(
 *     Equal)), which is not a total order: its result depends on the sort implementation.  Here NaN sorts after
 *     every number and before nulls, in both directions, and NaNs tie among themselves.
 * Errors: a U32CODE key without code_rank, or a code >= n_codes (checked on the device, no fault):
 * PANDRS_HIP_ERR_INVALID_ARGUMENT; fewer rows than min_size_threshold: PANDRS_HIP_ERR_BELOW_THRESHOLD; n_rows == 0:
 * OK, nothing written; n_rows >= 2^32: PANDRS_HIP_ERR_INVALID_ARGUMENT; ctx NULL (no context could be created, e.g.
 * no device): PANDRS_HIP_ERR_NOT_INITIALIZED.  The workspace (about 24 bytes per row, plus
 * 8 per row for every further 64 bits of concatenated key codes) is sized up front: a memory_limit below it is
 * PANDRS_HIP_ERR_OUT_OF_MEMORY.  Host key columns are staged; device / resident columns are read in place.  out_idx
 * (n_rows int64 row indices, the element type of the gathers) lives in out_mem_space.  The frame a sort returns is
 * select_rows_by_indices_impl (src/optimized/split_dataframe/select.rs:172-226): every column gathered through
 * out_idx with nulls as 0 / 0.0 / "" / false and no null masks (pandrs_hip_gather_column).
 * pandrs_hip_get_timings' n_partitions is the number of radix passes.  Each key becomes a code of bitlength(span + has_nan +
 * has_null) bits, span = max - min of its order-preserving images: image - min ascending, max - image descending, NaN =
 * span + 1, null = span + 1 + has_nan.  The codes are packed MSB-first, the last key at bit 0, into 64-bit words.  Per word,
 * the bits from the lowest to the highest one that varies over the rows are cut into ceil(bits / D) digits of ceil(bits /
 * digits) bits (D = 8, or "sort_digit_bits"); a digit takes a pass iff one of its bits varies.  All keys constant: 0 passes. */
int32_t pandrs_hip_sort_indices(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *keys, int32_t n_keys,
                                const int32_t *ascending, const uint32_t *code_rank, int64_t n_codes, int64_t n_rows,
                                int32_t out_mem_space, int64_t *out_idx);

/* ---- filter (stream compaction) ----------------------------------------------------------------------------
 * OptimizedDataFrame::filter (src/optimized/split_dataframe/data_ops.rs:37-121), filter_rows (row_ops.rs:26-130),
 * par_filter (parallel.rs:21-230) and select_by_mask (select.rs:150-167).  Two calls, in the shape of the join's retained
 * pairs (pandrs_hip_join_indices -> pandrs_hip_join_gather):
 *
 * pandrs_hip_filter_indices: the selection.  cond is a BOOLBITS column of n_rows rows, with or without a null mask.  Row i is
 * selected iff its value is Some(true) (the reference's `if let Ok(Some(true)) = bool_col.get(i)`): value bit set and
 * null bit clear; a null row is never selected.  *out_count = the number of selected rows; out_idx (when not NULL) receives
 * them as ascending int64 row indices, the element type every gather takes, in out_mem_space (room for *out_count
 * elements; n_rows is always enough).  out_idx NULL = the count only.  The context keeps the selection (the condition
 * as 64-bit words and one output offset per 4096-row tile) until the next pandrs_hip_filter_indices on it.
 *
 * pandrs_hip_filter_gather: one column compacted through the retained selection.  out (in out_mem_space) receives the
 * selected rows' values in row order, *out_count of the last filter_indices elements: I64 / F64 as 8 bytes, U32CODE
 * (string-pool codes) as 4, BOOLBITS as one 0 / 1 byte per row (as pandrs_hip_gather_column).  A null source cell becomes
 * fill_bits (data_ops.rs writes 0 / 0.0 / String::new() / false: the caller passes 0, the bits of 0.0, the pool code of
 * "" or 0), and the output has no null mask.  The source is streamed once; no index array is read.
 *
 * Both: host columns are staged; device / resident columns are read in place.
 * Errors: ctx NULL (no context could be created, e.g. no device): PANDRS_HIP_ERR_NOT_INITIALIZED; fewer rows than
 * min_size_threshold: PANDRS_HIP_ERR_BELOW_THRESHOLD; a condition that is not BOOLBITS: PANDRS_HIP_ERR_TYPE_MISMATCH
 * (data_ops.rs:115 ColumnTypeMismatch); n_rows >= 2^32: PANDRS_HIP_ERR_INVALID_ARGUMENT; filter_gather with no retained
 * selection, with n_src different from the selection's row count, or with a CELL64 column: PANDRS_HIP_ERR_INVALID_ARGUMENT.
 * n_rows == 0: OK, count 0 (a selection of 0 rows is retained).  The selection's workspace (n_rows / 8 bytes plus 8 bytes
 * per 4096-row tile) is sized up front, as is the staging of host columns (their bytes, plus n_rows * 8 for a host out_idx,
 * or the selected rows' bytes for a host out): a memory_limit below either is PANDRS_HIP_ERR_OUT_OF_MEMORY. */
int32_t pandrs_hip_filter_indices(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *cond, int64_t n_rows,
                                  int32_t out_mem_space, int64_t *out_idx, int64_t *out_count);
int32_t pandrs_hip_filter_gather(pandrs_hip_ctx *ctx, int32_t src_mem_space, const pandrs_hip_column *src, int64_t n_src,
                                 uint64_t fill_bits, int32_t out_mem_space, void *out);

/* ---- window statistics (rolling / expanding / EWM) -----------------------------------------------------------------
 * DataFrameWindowExt::{rolling, expanding, ewm} (src/dataframe/window.rs:13-160) over src/series/window.rs: Rolling
 * (:163-200 bounds, ops :206-345), Expanding (:379-400, ops :404-500), EWM (:608 get_alpha, :640-724).
 *
 * pandrs_hip_window: one statistic of one numeric column of n_rows rows.  col is I64 (cells `as f64`) or F64, with or
 * without a null mask (a null cell is the reference's None).  out (in out_mem_space) receives n_rows doubles; NaN marks a
 * None, and count is written as f64 (enhanced_window.rs).  The spec:
 *   kind  ROLLING: row i covers [max(0, i+1-window), i+1); center = 1: start = i >= window/2 ? i - window/2 : 0,
 *                  end = min(start + window, n) (so the first windows are [0, window), not a symmetric cut).
 *                  window >= 1 (window.rs:112-117); min_periods < 0 means window (:146).
 *         EXPANDING: row i covers [0, i+1); min_periods >= 0, taken as given (0 allowed).
 *         EWM:   alpha resolved by the caller (get_alpha, :608: alpha, 2/(span+1) or 1 - exp(-ln2/halflife)); it must be
 *                finite; adjust / ignore_na / ddof are never read by the reference and are not part of the spec.
 *   op    SUM / MEAN / VAR / STD / MIN / MAX / COUNT for ROLLING and EXPANDING; MEAN / STD / VAR for EWM.
 * Rolling and expanding: the window's values are its non-null cells in row order; fewer than min_periods -> NaN (count:
 * 0).  Otherwise sum = the left fold from -0.0 (current Rust std's `Sum for f64`), mean = sum / len, var = NaN when
 * len <= ddof, else mean as above and sum of (x-mean)*(x-mean) in row order / (len-ddof), std = sqrt(var),
 * min / max = fold(+-INFINITY, f64::min / max) (NaN cells ignored, a window of only NaN gives +-inf), count = len.
 * EWM mean: NaN until the first non-null value, which is output as itself, then y = alpha*v + (1-alpha)*y; a null row
 * repeats y.  EWM std: NaN up to and including the first value, then with diff = v - mean_prev,
 * var = (1-alpha)*(var + alpha*diff*diff), output sqrt(var); a null row repeats it.  EWM var = the std output squared
 * (:715-724, not the internal var).
 *
 * Parity.  Bit for bit: rolling sum / mean / var / std at every window (the same fold, in the same
 * order, no contraction; sqrt and f64 division are correctly rounded on the device), rolling and expanding min / max /
 * count, EWM rows before the first carried-in value.  Deviations:
 *  - min / max over values mixing +0.0 and -0.0: -0.0 < +0.0 (IEEE total order); f64::min leaves that tie unspecified;
 *  - expanding sum / mean: a compensated (double-double) parallel prefix, within 1e-9 * sum|x| of the row-order prefix
 *    (the sign of a zero sum is kept: a window of only -0.0, or an empty one under min_periods 0, sums to -0.0);
 *  - expanding var / std: Chan et al.'s merge of (count, mean, M2), within 1e-9 relative of the two-pass restatement,
 *    with an absolute floor of 1e-12 * max|x|^2 for var (1e-6 * max|x| for std) over the rows so far;
 *  - EWM mean / std / var: affine scans, then each thread re-runs the reference's recurrence from its carried-in value;
 *    within 1e-12 * max|x| over the rows so far (var, the std output squared: 2e-12 * max|x|^2).
 * Host columns are staged; device and resident columns are read in place (data 8-byte aligned; a null mask at any byte
 * offset).  Errors: ctx NULL: PANDRS_HIP_ERR_NOT_INITIALIZED; fewer rows than min_size_threshold:
 * PANDRS_HIP_ERR_BELOW_THRESHOLD; a column that is not I64 / F64: PANDRS_HIP_ERR_TYPE_MISMATCH; a bad spec (kind, op for
 * the kind, window < 1, center not 0 / 1, ddof < 0, expanding min_periods < 0, a non-finite alpha) or n_rows >= 2^32:
 * PANDRS_HIP_ERR_INVALID_ARGUMENT.  n_rows == 0: OK, nothing written.  Workspace is sized up front (rolling min / max /
 * count: 16 bytes per row, + 8 with a null mask; EWM std / var: 1 byte per row; staging: the host column and out): a
 * memory_limit below it is PANDRS_HIP_ERR_OUT_OF_MEMORY.  Median and quantile: pandrs_hip_window_quantile below.
 * Out of scope: apply (series/window.rs), the `closed` option (accepted by the reference, never read). */
typedef enum pandrs_hip_window_kind {
    PANDRS_HIP_WINDOW_KIND_ROLLING = 0,
    PANDRS_HIP_WINDOW_KIND_EXPANDING = 1,
    PANDRS_HIP_WINDOW_KIND_EWM = 2
} pandrs_hip_window_kind;

typedef enum pandrs_hip_window_op {
    PANDRS_HIP_WINDOW_SUM = 0,
    PANDRS_HIP_WINDOW_MEAN = 1,
    PANDRS_HIP_WINDOW_VAR = 2,
    PANDRS_HIP_WINDOW_STD = 3,
    PANDRS_HIP_WINDOW_MIN = 4,
    PANDRS_HIP_WINDOW_MAX = 5,
    PANDRS_HIP_WINDOW_COUNT = 6
} pandrs_hip_window_op;

typedef struct pandrs_hip_window_spec {
    int32_t kind;           /* pandrs_hip_window_kind */
    int32_t op;             /* pandrs_hip_window_op */
    int64_t window;         /* ROLLING: window_size >= 1 */
    int64_t min_periods;    /* ROLLING: < 0 = window; EXPANDING: >= 0 */
    int32_t center;         /* ROLLING: 0 / 1 */
    int32_t reserved;
    int64_t ddof;           /* VAR / STD of ROLLING and EXPANDING: >= 0 */
    double alpha;           /* EWM */
} pandrs_hip_window_spec;

int32_t pandrs_hip_window(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows,
                          const pandrs_hip_window_spec *spec, int32_t out_mem_space, double *out);

/* ---- window order statistics (rolling / expanding median and quantile) ---------------------------------------------------
 * Rolling::{median, quantile} (src/series/window.rs:298-336) and Expanding::{median, quantile} (:494-530) over the window
 * bounds of :163-203 / :379-400, as DataFrameRollingOps / DataFrameExpandingOps::{median, quantile} call them
 * (dataframe/enhanced_window.rs:283-290, :464-471), and PandasCompatExt::rolling_median (pandas_compat/functions.rs:2055 over
 * helpers/window_ops.rs:206-240).
 *
 * pandrs_hip_window_quantile: one order statistic of one numeric column of n_rows rows.  col is I64 (cells `as f64`) or
 * F64, with or without a null mask.  out (in out_mem_space) receives n_rows doubles.  Window bounds, min_periods and center
 * are pandrs_hip_window's (kind ROLLING or EXPANDING; EWM has no order statistic: PANDRS_HIP_ERR_INVALID_ARGUMENT).
 *   Window values: the window's included cells: non-null (window.rs:192, :390), and with nan_missing = 1 also non-NaN
 *     (window_ops.rs:221).  len = their number.  len < min_periods -> NaN (window.rs:194-199, :392-397).
 *   Sorted order: ascending by value, -0.0 and +0.0 tied, ties in row order: the reference's stable
 *     sort_by(partial_cmp) (window.rs:301, :326).
 *   Median (median = 1, q ignored): mid = len / 2; odd len: sorted[mid]; even len: (sorted[mid-1] + sorted[mid]) / 2.0
 *     (:302-307): one add and one divide, an overflow to +-inf is kept.
 *   Quantile (median = 0): idx = min(round(q * (len-1) as f64), len-1) with Rust's round (half away from zero), the result
 *     is sorted[idx] (:327-328).  q outside [0, 1]: PANDRS_HIP_ERR_INVALID_ARGUMENT (:318-322).
 * Parity: bit for bit at every window size, signed zeros included: the result is a cell of the column or the exact mean
 * of two.  Deviations:
 *  - len == 0 (possible under min_periods 0) gives NaN; the reference underflows `mid - 1` / `len - 1` and panics;
 *  - a NaN q is rejected; the reference's comparisons let it through and `NaN as usize` selects index 0;
 *  - with nan_missing = 0 a window that holds a NaN value gives NaN; the reference sorts it with a comparator that is not
 *    a total order, so its answer depends on the sort's internals.
 * Two paths give the same bits ("window_quantile_path" forces either): rolling windows of at most 44 rows select in LDS
 * with no workspace; every other window goes through the column's stable sort order (pandrs_hip_sort_indices' workspace
 * and 8 bytes per row) and a wavelet matrix over the sort ranks (16 bytes per row, + 16 bytes per 64 rows for each of the
 * bit-length-of-(n_rows-1) levels and two more).  Host columns are staged; device and resident columns are read in place
 * (data 8-byte aligned; a null mask at any byte offset).  Errors: ctx NULL: PANDRS_HIP_ERR_NOT_INITIALIZED; fewer rows than
 * min_size_threshold: PANDRS_HIP_ERR_BELOW_THRESHOLD; a column that is not I64 / F64: PANDRS_HIP_ERR_TYPE_MISMATCH; a bad
 * spec (kind, median / nan_missing / center not 0 / 1, window < 1, expanding min_periods < 0, q) or n_rows >= 2^32:
 * PANDRS_HIP_ERR_INVALID_ARGUMENT.  n_rows == 0: OK, nothing written.  The workspace is sized up front: a memory_limit below
 * it is PANDRS_HIP_ERR_OUT_OF_MEMORY.  pandrs_hip_get_timings: the direct path is PANDRS_HIP_PHASE_OTHER; the general path
 * shows the sort's phases, the ranks and levels as PANDRS_HIP_PHASE_BUILD and the queries as PANDRS_HIP_PHASE_PROBE. */
typedef struct pandrs_hip_window_quantile_spec {
    int32_t kind;           /* PANDRS_HIP_WINDOW_KIND_ROLLING or _EXPANDING */
    int32_t median;         /* 1: median (q ignored); 0: quantile(q) */
    int64_t window;         /* ROLLING: window_size >= 1 */
    int64_t min_periods;    /* ROLLING: < 0 = window; EXPANDING: >= 0 */
    int32_t center;         /* ROLLING: 0 / 1 */
    int32_t nan_missing;    /* 0: only null cells are missing (series/window.rs); 1: NaN cells too (window_ops.rs:221) */
    double q;               /* quantile: 0 <= q <= 1 */
} pandrs_hip_window_quantile_spec;

int32_t pandrs_hip_window_quantile(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows,
                                   const pandrs_hip_window_quantile_spec *spec, int32_t out_mem_space, double *out);

/* ---- describe and exact percentiles of one numeric column ------------------------------------------------------------------
 * Replaces OptimizedDataFrame::describe / describe_all (src/optimized/split_dataframe/stats.rs:50-171) over stats::describe
 * and percentile (src/stats/descriptive.rs:91-166, :169-200), and the quantile part that describe_gpu
 * (src/stats/gpu.rs:240-316) leaves to a CPU sort.  The values are the column's non-null cells as f64 (`v as f64` for I64):
 *   count            the non-null cells;
 *   mean             sum / count (:102);
 *   std              sqrt(sum (x - mean)^2 / (count - 1)), two passes (:107-108); count == 1 gives 0.0 / 0.0 = NaN;
 *   min, max         sorted[0], sorted[count - 1] (:110-111);
 *   percentile p     index = (p / 100.0) * (count - 1) as f64, lo = floor, hi = ceil; sorted[lo] when lo == hi, else
 *                    sorted[lo] * (1.0 - w) + sorted[hi] * w with w = index - lo; p == 0 and p == 100 are the ends (:182-199).
 * pandrs_hip_describe is pandrs_hip_quantiles at 25 / 50 / 75 plus the moments in one call: the column is read once per pass,
 * not once per statistic.  How: no sort; a multi-rank most-significant-digit radix SELECT (describe.hip): one stream for
 * the counts, the sum and the extreme order-preserving codes, then one stream per 8-bit digit of (code - min code) that
 * varies, counting only the rows that still match a wanted rank's prefix; the first of them also carries sum (x - mean)^2.
 * Geometry (tests read it): describe_tile_rows = 2048 rows per workgroup iteration, describe_blocks_per_cu = 4, grid =
 * min(describe_blocks_per_cu x compute units, ceil(n_rows / describe_tile_rows)) workgroups striding over the tiles.
 * Exactness: min, max and every percentile are bit for bit the reference's (the selected element is the element its sort
 * puts at that rank, also for I64 values beyond 2^53; the interpolation is the reference's expression, FMA contraction
 * off); count is exact; mean and std carry the bound of the other device sums: within 1e-9 relative of
 * the reference's sequential fold.
 * Deviations:
 *  - NaN: the reference's `partial_cmp(..).unwrap()` (:99) panics on a NaN cell.  Here a NaN cell counts and orders after
 *    every number, as in pandrs_hip_sort_indices: max, and every percentile whose rank reaches the NaN block, are NaN; min
 *    is the smallest number (NaN when there is none); mean and std are NaN by arithmetic.
 *  - Signed zero: the order is the order-preserving code's, -0.0 before +0.0 (the reference's comparison ties them and its
 *    stable sort keeps row order), so a result that is zero may differ from the reference in its sign bit only.
 *  - describe_all: the reference's `if let Ok` (stats.rs:157-171) leaves out a column on any error.  The mirrors leave out
 *    only a column whose describe raises InvalidValue (count 0 or 1); a device or argument error surfaces.
 * count == 0 (no row, or only nulls) is status OK with count 0 and NaN everywhere; the reference returns
 * Err(InvalidValue) (:92-96) and the mirrors raise it.  The reference also fails for count == 1 (its confidence interval
 * asks TDistribution::new(0.0), src/stats/distributions.rs:188-193: Err(InvalidValue)); the ABI answers such a column
 * (std NaN), the mirrors raise.
 * Host columns are staged; device and resident columns are read in place (data 8-byte aligned, 16-byte alignment not
 * needed; a null mask at any byte offset, bits past n_rows ignored).  The workspace does not grow with n_rows (per-workgroup
 * partials, 32 x 256 digit counts, the rank slots); staging: the host column.  A memory_limit below either is
 * PANDRS_HIP_ERR_OUT_OF_MEMORY.  Errors: ctx NULL: PANDRS_HIP_ERR_NOT_INITIALIZED; fewer rows than min_size_threshold:
 * PANDRS_HIP_ERR_BELOW_THRESHOLD; a column that is not I64 / F64: PANDRS_HIP_ERR_TYPE_MISMATCH; a NULL pointer, n_rows >=
 * 2^32, n_percentiles outside 1 .. 16, a percentile outside [0, 100] or NaN (:176-180): PANDRS_HIP_ERR_INVALID_ARGUMENT.
 * Out of scope: mode, confidence intervals and outliers of StatisticalSummary (skewness and kurtosis: pandrs_hip_moments). */
typedef struct pandrs_hip_describe_stats {
    int64_t count;          /* non-null cells */
    double mean, std, min, q1, median, q3, max;   /* NaN each when count == 0 */
} pandrs_hip_describe_stats;

int32_t pandrs_hip_describe(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows,
                            pandrs_hip_describe_stats *out);

/* percentile(sorted non-null values, p) for 1 .. 16 values of p in [0, 100], any order, repeats allowed; out[j] answers
 * percentiles[j], out_count = the non-null cells.  percentiles / out / out_count are host pointers. */
int32_t pandrs_hip_quantiles(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows,
                             const double *percentiles, int32_t n_percentiles, double *out, int64_t *out_count);

/* ---- shape statistics of whole columns: fused sums of 1 .. 16 columns ---------------------------------------------------------------
 * Replaces the whole-column statistics of PandasCompatExt that are a few sums over the column: skew / kurtosis
 * (src/dataframe/pandas_compat/functions.rs:1617-1665), sem / mad / prod / cv / geometric_mean / harmonic_mean
 * (src/dataframe/pandas_compat/helpers/aggregations.rs:8-51, :108-139, :162-181), var_column / std_column (functions.rs:3571-3588),
 * range / abs_sum (:4207-4224), the sums behind zscore (:2284-2314) and describe_column (aggregations.rs:54-81), and the per-frame
 * lists sum_all / mean_all / std_all / var_all / min_all / max_all (:934-1022) and product_all (:1583-1595).  The mirrors restate
 * each reference expression on the host over the fields below; this entry computes the fields.
 * The cells that count are neither null nor NaN (every reference function here filters `!v.is_nan()`; a null cell is the
 * mirrors' missing value), taken as f64 (`v as f64` for I64).  A field whose `want` bit is clear is NaN.
 * How (moments.hip): the grid is (workgroups, columns); the number of launches does not depend on n_cols.
 *  1. the first stream (pandrs_hip_describe's: a thread's rows depend on row numbers only) gives the counts, sum, abs_sum, min and
 *     max, and - only in the kernel variant the `want` bits select - log_sum, recip_sum and prod.  ln and the IEEE divide cost
 *     tens of f64 instructions per row; a call that asks for none of WANT_LOG / WANT_RECIP / WANT_PROD runs the lean variant.
 *  2. WANT_CENTRAL only: every workgroup folds its column's partials of step 1 in one fixed order, so all of them hold the
 *     same bits of mean (a launch-boundary reduce with no launch of its own), then one more stream gives m2, m3, m4 and abs_dev
 *     together: the column is read twice for all central statistics, not once per statistic.
 *  3. a small finish kernel folds the partials in that order and writes the structs.
 * No float atomics anywhere: a result is the same run to run and the same for a host, a device and a resident column.
 * Geometry (tests read it): moments_tile_rows = 2048 rows per workgroup iteration, moments_blocks_per_cu = 4,
 * moments_max_columns = 16, grid = (min(moments_blocks_per_cu x compute units, ceil(n_rows / moments_tile_rows)), n_cols)
 * workgroups of 256 threads, each striding over its column's tiles.
 * Exactness: the counts, min and max are exact, bit for bit (min / max through the order-preserving code of the f64 value).
 * mean is sum / count of the returned fields, exactly; the central sums are taken around that mean.  Every sum S = sum t_i
 * (sum, abs_sum, log_sum, recip_sum, m2, m3, m4, abs_dev) is a parallel fold: with u = 2^-53, gamma_m = m u / (1 - m u) and m =
 * count, |got - ref| <= (2 gamma_m + 4 u) sum |t_i| against the reference's sequential fold of the same terms (both folds lie
 * within gamma_m sum |t| of the true sum, as for pandrs_hip_cumulative SUM; a term may round differently by a few ulps: `powi`
 * against multiplication, the device's ln at 1 ulp against libm).  Integer-valued cells whose mean is an integer and whose
 * sums stay below 2^53: bit for bit; cells that are +- powers of two: recip_sum and prod bit for bit.
 * prod: the (mantissa, exponent) state of pandrs_hip_cumulative PROD (frexp / ldexp; 0, +-inf and NaN stay in the mantissa,
 * where IEEE multiplication gives the reference's class and sign), converted once at the end.  Same contract: wherever every
 * reference running product is normal, zero by a zero input, infinite by an infinite input, or NaN, the relative error is at
 * most 2 gamma_m and class and sign are exact.  Same deviation: the reference's sequential fold is sticky after a range
 * excursion of finite nonzero inputs ([1e200, 1e200, 1e-200, 1e-200] is +inf there); the whole-column product here is the value
 * the extended-range product rounds to (1.0 for that column), whatever the order of the cells.
 * Deviations:
 *  - Signed zero: min and max order -0.0 before +0.0 (pandrs_hip_describe); f64::min / f64::max leave the sign of a zero tie to
 *    the order of the cells, so a min or max that is zero may differ from the reference in its sign bit only.
 *  - Null cells: the reference's get_column_numeric_values returns Err on a missing value; here a null cell is skipped like NaN.
 * n_rows == 0 is status OK: the counts 0, sum and every wanted sum -0.0 (Rust's Sum for f64 starts there), min +inf, max -inf
 * (the fold identities), prod 1.0, mean NaN.  A column of only null or NaN cells gives the same.
 * Host columns are staged; device and resident columns are read in place (data 8-byte aligned; a data pointer 8 bytes off a
 * 16-byte boundary takes its row pairs as two 8-byte loads; each column its own optional null mask at any byte offset, bits
 * past n_rows ignored).  Workspace: 88 + 32 bytes per (workgroup, column) and the structs; it does not grow with n_rows.
 * Staging: the host columns.  A memory_limit below either is PANDRS_HIP_ERR_OUT_OF_MEMORY.
 * pandrs_hip_get_timings: the phase is PANDRS_HIP_PHASE_AGGREGATE; n_partitions names the first stream's variant, 1 + (LOG ? 1 : 0)
 * + (RECIP ? 2 : 0) + (PROD ? 4 : 0), so 1 is the lean one; table_slots is the number of streams (1, or 2 with WANT_CENTRAL).
 * Errors: ctx NULL: PANDRS_HIP_ERR_NOT_INITIALIZED; fewer rows than min_size_threshold: PANDRS_HIP_ERR_BELOW_THRESHOLD; a column
 * that is not I64 / F64: PANDRS_HIP_ERR_TYPE_MISMATCH; a NULL pointer, n_cols outside 1 .. 16, n_rows < 0 or >= 2^32, unknown
 * `want` bits: PANDRS_HIP_ERR_INVALID_ARGUMENT.
 * Out of scope: skew / kurtosis as groupby aggregates, corr / cov, mode, confidence intervals. */
#define PANDRS_HIP_MOMENTS_MAX_COLUMNS 16
#define PANDRS_HIP_MOMENTS_WANT_CENTRAL 1     /* mean's second stream: m2, m3, m4, abs_dev */
#define PANDRS_HIP_MOMENTS_WANT_LOG 2         /* log_sum */
#define PANDRS_HIP_MOMENTS_WANT_RECIP 4       /* recip_sum */
#define PANDRS_HIP_MOMENTS_WANT_PROD 8        /* prod */
typedef struct pandrs_hip_moments_stats {
    int64_t count;          /* cells that are neither null nor NaN (the reference's `valid`) */
    int64_t count_pos;      /* of them > 0      (geometric_mean's filter, aggregations.rs:110-114) */
    int64_t count_nonzero;  /* of them != 0.0   (harmonic_mean's filter, :127-131) */
    double sum, abs_sum;    /* sum x, sum |x| */
    double min, max;        /* f64::min / f64::max folds from +inf / -inf */
    double mean;            /* sum / count, the value the central sums were taken around */
    double m2, m3, m4;      /* sum (x - mean)^2, ^3, ^4          (WANT_CENTRAL) */
    double abs_dev;         /* sum |x - mean|                     (WANT_CENTRAL) */
    double log_sum;         /* sum ln x over x > 0                (WANT_LOG) */
    double recip_sum;       /* sum 1.0 / x over x != 0            (WANT_RECIP) */
    double prod;            /* product of the valid cells from 1.0 (WANT_PROD) */
} pandrs_hip_moments_stats;

/* cols: n_cols columns of n_rows rows each; out: n_cols structs on the host, out[i] answers cols[i]. */
int32_t pandrs_hip_moments(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *cols, int32_t n_cols, int64_t n_rows,
                           uint32_t want, pandrs_hip_moments_stats *out);

/* ---- order statistics by the reference's index rules, and the trimmed mean -------------------------------------------------------
 * Replaces the sorts of PandasCompatExt::iqr, describe_column's quartiles, percentile_value and trimmed_mean
 * (src/dataframe/pandas_compat/helpers/aggregations.rs:83-102, :142-159, :184-225) and of median_all
 * (src/dataframe/pandas_compat/functions.rs:1597-1615).  The reference indexes its sorted `valid` vector, the m cells that are
 * neither null nor NaN, four ways; none of them is pandrs_hip_quantiles' interpolation:
 *   AT_FRAC_N      sorted[(usize)(m * a)], NaN when that index is m or more (`get(..).unwrap_or(NAN)`; :87-89, :152-153);
 *   AT_FRAC_N1     sorted[(usize)((m - 1) * a)] (:198); a outside [0, 1] is NaN (the early return at :185);
 *   MEDIAN         (sorted[m/2 - 1] + sorted[m/2]) / 2.0 for even m, else sorted[m/2] (functions.rs:1604-1609); its arg is ignored;
 *   TRIMMED_MEAN   the mean of sorted[t .. m - t), t = (usize)(m * a) (:217-224); a outside [0, 0.5) is NaN (the early return at
 *                  :204), as is an empty slice (:220-222).
 * Counting rule: m counts the cells that are neither null nor NaN - unlike pandrs_hip_describe, where NaN cells count and
 * sort last.  out_count = m.  m == 0 is status OK with NaN results.
 * How (describe.hip): pandrs_hip_describe's radix select with "ranks by number": the ranks depend on m, which the host does
 * not know before the first stream, so the one-workgroup ranks kernel evaluates each op's rule on the device from the counts of
 * that stream, in double as the reference does.  Two ranks per op at the most, so the 1 .. 8 ops of a call never need more than
 * the select's 32 slots.  TRIMMED_MEAN selects v_lo = sorted[t] and v_hi = sorted[m - 1 - t], then runs one band stream over
 * the column: the sum of the cells whose order code lies strictly between the two selected codes, and the numbers of cells
 * below, on the lower code, on the upper code and above.  The finish adds (n_below + n_eq_lo - t) x v_lo + (n_eq_hi + n_above -
 * t) x v_hi - or (m - 2t) x v_lo when both ranks select one code - and divides by m - 2t, so ties at either cut count exactly as
 * often as the sorted slice holds them.  The early returns for `a` are decided on the host before any launch.
 * Geometry: pandrs_hip_describe's (describe_tile_rows, describe_blocks_per_cu); one band stream per TRIMMED_MEAN op.
 * Exactness: every selected value is bit for bit the element the reference's sort puts at that rank (also I64 beyond 2^53:
 * the integer is selected, then converted); MEDIAN's and the trimmed mean's arithmetic is the expression above, FMA contraction
 * off.  The band sum is a parallel fold: |got - ref| <= (2 gamma_k + 4 u) sum |x| over the band's k cells, divided by m - 2t;
 * integer-valued cells with sums below 2^53: bit for bit.  Deviation: signed zero orders -0.0 before +0.0, as documented for
 * pandrs_hip_describe.
 * Host columns are staged; workspace: pandrs_hip_describe's plus 8 x 40 bytes per workgroup; it does not grow with n_rows.
 * pandrs_hip_get_timings: n_partitions is the number of band streams run.
 * Errors: as pandrs_hip_describe (NOT_INITIALIZED, BELOW_THRESHOLD, TYPE_MISMATCH, OUT_OF_MEMORY); a NULL pointer, n_rows < 0 or
 * >= 2^32, n_ops outside 1 .. 8 (more ranks than the select's slots), an unknown op, a NaN `a` (MEDIAN's excepted):
 * PANDRS_HIP_ERR_INVALID_ARGUMENT.
 * Out of scope: quantile / percentile with interpolation (functions.rs:735; pandrs_hip_quantiles), mode. */
#define PANDRS_HIP_ORDER_STATS_MAX_OPS 8
typedef enum pandrs_hip_order_stat {
    PANDRS_HIP_OS_AT_FRAC_N = 0, PANDRS_HIP_OS_AT_FRAC_N1 = 1, PANDRS_HIP_OS_MEDIAN = 2, PANDRS_HIP_OS_TRIMMED_MEAN = 3
} pandrs_hip_order_stat;

/* ops / args / out: n_ops entries each on the host, out[j] answers (ops[j], args[j]); out_count = m. */
int32_t pandrs_hip_order_stats(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows,
                               const int32_t *ops, const double *args, int32_t n_ops, double *out, int64_t *out_count);

/* ---- rank of one numeric column ---------------------------------------------------------------------------------------------
 * PandasCompatExt::rank(column, RankMethod) (src/dataframe/pandas_compat/functions.rs:193-236, RankMethod at
 * pandas_compat/types.rs:48-59, known answer functions.rs:4393-4404): out[i], i in [0, n_rows), = the rank of row i, ascending
 * and 1-based.  The m rankable cells are taken in ascending STABLE order (the reference's sort_by is stable); a tie run
 * occupies the 0-based positions [s, e):
 *   AVERAGE  (s + e + 1) / 2.0          MIN  s + 1          MAX  e
 *   FIRST    position + 1: ties rank in original row order          DENSE  the 1-based number of the run.
 * Ties are the reference's `==` (:202): for F64 numeric equality, so -0.0 ties 0.0, as in pandrs_hip_sort_indices.  Every
 * result is an integer or half-integer below 2^33 built from integers: bit for bit the reference's, whatever the memory space.
 * col is I64 or F64, with or without a null mask; any other dtype: PANDRS_HIP_ERR_TYPE_MISMATCH.
 * How (rank.hip): pandrs_hip_sort_indices' stable radix sort leaves the permutation on the device (NaN after every number,
 * nulls after NaN); one pass over sorted positions marks where a tie run starts (the cell differs from its predecessor's; the
 * cells themselves are compared) as one bit per position, with every tile's number of starts and its first and last one; one
 * small workgroup carries the open run and the start count in from the tiles to the left and the next start in from the right
 * (two levels, every hand-off a kernel boundary); a last pass turns each position into its run's start, end and dense number
 * and writes out[perm[p]].  FIRST needs no boundaries, DENSE no run ends.
 * Geometry (tests read it): rank_tile_rows = 2048 sorted positions per workgroup iteration, rank_blocks_per_cu = 4, grid =
 * min(rank_blocks_per_cu x compute units, ceil(n_rows / rank_tile_rows)) workgroups striding over the tiles.
 * Deviations:
 *  - NaN and null: the reference never terminates on a NaN cell (at :202 the inner `while` does not advance because NaN ==
 *    NaN is false, and `i = j` repeats) and returns Err(InvalidValue) on a missing value (src/dataframe/base.rs:555-561).
 *    Here a NaN cell and a null cell get rank NaN and take no rank (pandas' na_option="keep"); the m rankable cells are
 *    ranked 1 .. m.
 *  - I64: the reference casts to f64 (base.rs:569), which ties neighbours beyond 2^53 and leaves their FIRST order to row
 *    order.  Here I64 cells are compared as integers, exactly: the position pandrs_hip_describe takes for I64 order statistics.
 * Host columns are staged; device and resident columns are read in place (data and out 8-byte aligned; a null mask at any
 * byte offset, bits past n_rows ignored); out (n_rows doubles) lives in out_mem_space.  pandrs_hip_get_timings' n_partitions
 * is the number of radix passes, as for the sort (0 when every cell is equal); the rank phase is PANDRS_HIP_PHASE_AGGREGATE.
 * Workspace, sized up front: pandrs_hip_sort_indices' for one key (24 bytes per row, plus 8 per row for a code beyond 64 bits: a
 * full-range I64 column with a null has a 65-bit code) plus, for the rank phase, 8 bytes per row (the permutation) and 1 / 8
 * byte per row plus 24 bytes per rank_tile_rows rows (start bits and tile summaries): 32.2 bytes per row for a code of up to
 * 64 bits; staging: the host column and a host out.  A memory_limit below either is PANDRS_HIP_ERR_OUT_OF_MEMORY.
 * Errors: ctx NULL: PANDRS_HIP_ERR_NOT_INITIALIZED; fewer rows than min_size_threshold: PANDRS_HIP_ERR_BELOW_THRESHOLD; a NULL
 * col / out, a method outside 0 .. 4 or n_rows >= 2^32: PANDRS_HIP_ERR_INVALID_ARGUMENT.  n_rows == 0: OK, nothing written.
 * Out of scope: a descending order, pct, a grouped rank, rank through the legacy string frame (nlargest / nsmallest are
 * pandrs_hip_topk, below), and
 * OptimizedDataFrame::mann_whitney_u (split_dataframe/stats.rs:332: its ties are a chained |a - b| < EPSILON, not equality, and
 * its p-value is an approximation of the reference's own). */
typedef enum pandrs_hip_rank_method {   /* RankMethod, types.rs:48-59, same order */
    PANDRS_HIP_RANK_AVERAGE = 0, PANDRS_HIP_RANK_MIN = 1, PANDRS_HIP_RANK_MAX = 2,
    PANDRS_HIP_RANK_FIRST = 3, PANDRS_HIP_RANK_DENSE = 4
} pandrs_hip_rank_method;

int32_t pandrs_hip_rank(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows,
                        int32_t method, int32_t out_mem_space, double *out);

/* ---- missing cells of one numeric column: ffill, bfill, interpolate, fillna -------------------------------------------------
 * PandasCompatExt::fillna (src/dataframe/pandas_compat/functions.rs:789), fillna_method (:811-868), interpolate (:870-918),
 * ffill / bfill (:3626-3683); known answers :4751-4970, :8007-8050.  A cell is MISSING when its null bit is set or, for an F64
 * column, when it is NaN (the reference's is_nan() marker); an I64 cell is missing only by its null bit.  Everything else is
 * valid: +-inf and -0.0 too.  A valid row's cell is copied unchanged.  For a missing row i:
 *   FFILL   the cell of the nearest valid row before i, bit for bit; a row with no valid row before it stays missing.
 *   BFILL   the mirror image: the nearest valid row after i.
 *   LINEAR  between the nearest valid rows p < i < q: a + ((b - a) * (double)(i - p)) / (double)(q - p), a and b the cells as
 *           f64 (`v as f64` for I64): the reference's expression (:889-894) in that association, every operation rounded on its
 *           own (no fused multiply-add).  Rows before the first or after the last valid row stay missing.  The output is F64
 *           whatever the column: a valid I64 cell is written as (double)v.
 *   VALUE   the 8-byte cell fill_bits, as is (an I64 value, or the bits of an f64).  An F64 fill_bits that is NaN leaves the
 *           rows missing, as the reference's fillna(NaN) does.
 * The output has the column's dtype except under LINEAR.  A row that stays missing is written as the canonical quiet NaN
 * 0x7FF8000000000000 for an F64 output and as 0 for an I64 output, and its bit is set in out_null_mask.  An interior LINEAR row
 * whose arithmetic gives NaN (inf - inf) is NOT missing: its bit is 0.  *out_n_missing = the rows still missing.
 * How (fill.hip): (1) one stream over the column and its mask writes one valid bit per row (a wave ballot is the 64-row word)
 * and every tile's first and last valid row; for I64 only the mask is read; (2) one small workgroup carries "the last valid row
 * to the left" and "the first valid row to the right" across the tile summaries, "none" kept apart from row 0 (row + 1 on the
 * left, 0xFFFFFFFF on the right); every hand-off between workgroups is a kernel boundary, no workgroup waits for another; (3) per
 * tile the words give each row its source (highest set bit at or below it / lowest set bit at or above it, else the carry), a
 * missing row gathers it (LINEAR: both ends) and the ballot of "still missing" is the output mask word.  VALUE is one kernel; an
 * I64 column without a mask has nothing missing and is copied (LINEAR: converted).
 * Geometry (tests read it): fill_tile_rows = 2048 rows per workgroup iteration, fill_blocks_per_cu = 4, grid =
 * min(fill_blocks_per_cu x compute units, ceil(n_rows / fill_tile_rows)) workgroups striding over the tiles.
 * Deviations:
 *  - the reference casts every numeric column to f64 (get_column_numeric_values) and has no null mask on this path: a missing
 *    value there is a NaN cell only.  Here a null bit counts as missing too, and the cell under it is never a source.
 *  - here I64 stays I64 under FFILL / BFILL / VALUE, exactly; only LINEAR answers in f64.
 * Buffers: col is I64 or F64, with or without a mask; any other dtype: PANDRS_HIP_ERR_TYPE_MISMATCH.  Host columns and outputs
 * are staged; device and resident columns are read in place.  Data and out_data are 8-byte aligned (16 is not required); the
 * masks may sit at any byte offset, input bits past n_rows are ignored.  out_data receives n_rows x 8 bytes.  out_null_mask
 * receives exactly ceil(n_rows / 8) bytes, bits past n_rows in the last byte 0, and no byte beyond is touched (the words are
 * stored bytewise); it may be NULL, except where the output is I64 and the column has a mask and the method is not VALUE (the
 * data alone could not tell a missing row from a 0): PANDRS_HIP_ERR_INVALID_ARGUMENT.  out_data or out_null_mask overlapping the
 * column's data or mask in the same memory space: PANDRS_HIP_ERR_INVALID_ARGUMENT (missing rows gather from their neighbours, so
 * the call cannot run in place).  out_n_missing is a host pointer and may be NULL.
 * pandrs_hip_get_timings: the phase is PANDRS_HIP_PHASE_AGGREGATE, n_partitions is 0, algorithmic_bytes counts the streams run.
 * Workspace, sized up front in one arena: n_rows / 8 bytes of valid bits plus 16 bytes per fill_tile_rows rows plus the counter:
 * about 0.13 bytes per row (VALUE and an unmasked I64 column: the counter only); staging: a host column and host outputs.  A
 * memory_limit below either is PANDRS_HIP_ERR_OUT_OF_MEMORY.
 * Errors: ctx NULL: PANDRS_HIP_ERR_NOT_INITIALIZED; fewer rows than min_size_threshold: PANDRS_HIP_ERR_BELOW_THRESHOLD; a NULL
 * col / out_data, a method outside 0 .. 3 or n_rows >= 2^32: PANDRS_HIP_ERR_INVALID_ARGUMENT.  n_rows == 0: OK, nothing written,
 * *out_n_missing = 0.
 * Out of scope: limit=, non-linear interpolation (dropna / isna / count_na: pandrs_hip_predicate, below), group-wise fills, String and Boolean columns, the
 * legacy string frame, TimeSeries::fillna_forward. */
typedef enum pandrs_hip_fill_method {
    PANDRS_HIP_FILL_FFILL = 0, PANDRS_HIP_FILL_BFILL = 1, PANDRS_HIP_FILL_LINEAR = 2, PANDRS_HIP_FILL_VALUE = 3
} pandrs_hip_fill_method;

int32_t pandrs_hip_fill(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows,
                        int32_t method, uint64_t fill_bits, int32_t out_mem_space, void *out_data, uint8_t *out_null_mask,
                        int64_t *out_n_missing);

/* ---- the first k rows of one numeric column in order: nlargest / nsmallest, idxmax / idxmin ----------------------------------
 * PandasCompatExt::nlargest / nsmallest (src/dataframe/pandas_compat/functions.rs:159-174) and idxmax / idxmin (:175-192); known
 * answers functions.rs:4369-4391.  One column, I64 or F64, with or without a null mask, n_rows rows, a direction and k >= 0.
 * The order O(direction) over ALL rows:
 *   1. the numbers by value, descending for LARGEST, ascending for SMALLEST: F64 by numeric comparison (-0.0 ties 0.0, as in
 *      pandrs_hip_sort_indices), I64 as integers, exactly;
 *   2. ties in ascending row order (the reference's sort_by is stable);
 *   3. then the NaN rows in ascending row order;  4. then the null rows in ascending row order.
 * NaN and null come last in BOTH directions.  pandrs_hip_topk writes the first min(k, n_rows) rows of O as int64 row indices to
 * out_rows (out_mem_space), *out_count = min(k, n_rows) and *out_n_numbers = how many of them are numbers: the numbers come
 * first, so a caller that drops the missing tail (pandas) cuts there.  As a property: out_rows equals the first k entries of
 * pandrs_hip_sort_indices on that one key with ascending = [direction == SMALLEST], index for index.
 * pandrs_hip_arg_extreme is idxmin and idxmax in one pass: out_rows[0] = the FIRST row that holds the minimum (Iterator::min_by
 * keeps the first of equals), out_rows[1] = the LAST row that holds the maximum (max_by keeps the last); NaN and null cells
 * are skipped; *out_found = 0 when the column holds no number (the reference's None for an empty column; out_rows untouched), else
 * 1.  The same ties: -0.0 equals 0.0, I64 as integers.
 * How (topk.hip): (1) one census stream gives the counts of numbers (m), NaN and null cells and the extreme order-preserving
 * codes with their rows (that is arg_extreme's whole kernel); the output is kn = min(k, m) numbers, then NaN rows, then null
 * rows; (2) a single-rank most-significant-digit radix select of rank kn - 1 over code - min (LARGEST: max - code), one stream
 * per 8-bit digit that varies, finds the threshold; kn == m needs none; (3) reduce-then-scan compaction: the rows better than
 * the threshold, equal to it, NaN and null are counted per tile, one workgroup scans the counts, and a last stream (tiles with
 * nothing to give are skipped) writes the s better rows to a candidate list, the first kn - s equal rows, NaN rows and null rows
 * to their final slots, all in row order by wave ballots; (4) s comes back to the host (ONE read-back of its own, 8 bytes of
 * state that size the next step; the nested sort then makes its own two), pandrs_hip_sort_indices' stable sort orders the s < k candidates and their row numbers are
 * gathered into out_rows[0, s).  Every hand-off between workgroups is a kernel boundary; no workgroup waits for another.
 * Geometry (tests read it): topk_tile_rows = 2048 rows per workgroup iteration, topk_blocks_per_cu = 4, grid =
 * min(topk_blocks_per_cu x compute units, ceil(n_rows / topk_tile_rows)) workgroups striding over the tiles.  Cut-over: from
 * topk_cutover = 1 / 5 on, i.e. when 5 * min(k, n_rows) >= 1 * n_rows, the column is sorted whole and the first k entries kept: the
 * earliest measured crossing of select and sort (a narrow-coded column at 100 M rows, docs/EXPERIMENT_LOG.md "Top-k"), rounded
 * towards the sort.  Both sides give the same output ("topk_path" forces either).
 * Deviations:
 *  - NaN: the reference's `partial_cmp(..).unwrap_or(Equal)` is no total order once a NaN cell is present, so its result is
 *    unspecified.  Here NaN rows are simply last, before the null rows, and arg_extreme skips them.
 *  - null: the reference reads a missing value as an error or as a number, depending on the frame; here a null row is last and the
 *    cell under its bit is never looked at.
 *  - I64: the reference casts to f64, which ties neighbours beyond 2^53; here I64 cells are compared as integers: the position
 *    pandrs_hip_rank and pandrs_hip_describe take.
 * Host columns are staged; device and resident columns are read in place (data and out_rows 8-byte aligned, 16 is not needed; a
 * null mask at any byte offset, bits past n_rows ignored).  out_rows receives exactly min(k, n_rows) entries and nothing beyond.
 * out_count, out_n_numbers, out_found and arg_extreme's out_rows are host pointers.  pandrs_hip_get_timings: the census and the
 * select are PANDRS_HIP_PHASE_OTHER, the compaction PANDRS_HIP_PHASE_SCATTER, the sort its own phases; n_partitions = the digit
 * streams of the select (above the cut-over: the sort's passes).
 * Workspace, sized up front: 56 bytes per workgroup, 256 digit counts, 32 bytes per topk_tile_rows rows (per-tile counts and
 * offsets of the four classes), 16 x min(k, n_rows) bytes of candidates, plus pandrs_hip_sort_indices' need for min(k, n_rows)
 * rows of one key with its permutation (32 bytes per row): 48 bytes per requested row and 1 / 64 byte per column row.  Above the
 * cut-over: the sort's 24 bytes per row (plus 8 for a code beyond 64 bits) and the permutation's 8.  arg_extreme: the 56 bytes per
 * workgroup.  Staging: the host column and a host out_rows.  A memory_limit below either is PANDRS_HIP_ERR_OUT_OF_MEMORY.
 * Errors: ctx NULL: PANDRS_HIP_ERR_NOT_INITIALIZED; fewer rows than min_size_threshold: PANDRS_HIP_ERR_BELOW_THRESHOLD; a column that
 * is not I64 / F64: PANDRS_HIP_ERR_TYPE_MISMATCH; a NULL col / out pointer, k < 0, a direction outside 0 .. 1 or n_rows >= 2^32:
 * PANDRS_HIP_ERR_INVALID_ARGUMENT.  n_rows == 0 or k == 0: OK, nothing written, both counts 0.
 * Out of scope: keep= variants, a multi-column nlargest, a grouped top-k, String and Boolean columns, the legacy string frame,
 * argmax / argmin / pct_rank, and rows beyond 2^32. */
typedef enum pandrs_hip_topk_direction { PANDRS_HIP_TOPK_LARGEST = 0, PANDRS_HIP_TOPK_SMALLEST = 1 } pandrs_hip_topk_direction;

int32_t pandrs_hip_topk(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows, int64_t k,
                        int32_t direction, int32_t out_mem_space, int64_t *out_rows, int64_t *out_count, int64_t *out_n_numbers);

int32_t pandrs_hip_arg_extreme(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows,
                               int64_t out_rows[2], int32_t *out_found);

/* ---- row masks of one column: compare, between, isna, isin ---------------------------------------------------------------------
 * PandasCompatExt::gt / ge / lt / le / eq_value / ne_value (src/dataframe/pandas_compat/helpers/comparison_ops.rs:7-46), between
 * (functions.rs:253-257), is_between (functions.rs:4141-4161), isna / notna (:930-933, :1312-1315), is_finite / is_infinite
 * (:4016-4024), isin / isin_numeric (functions.rs:141-158); known answers functions.rs:4362-4367, :4405-4410, :5007-5008,
 * :8121-8131, :8143-8147, :8348-8352, :8520-8524.  What filter / par_filter / select_by_mask consume, built where the column lives.
 * Output: out_bits is an LSB-first bitmap of ceil(n_rows / 8) bytes, bit = 1 the row is selected: the data of a BOOLBITS column
 * with no null mask, so pandrs_hip_filter_indices takes it in place.  out_bits may be NULL (the count only); *out_count = the
 * number of set bits (out_count may be NULL when out_bits is not).  Bits at and beyond n_rows in the last byte are 0; no byte at
 * or beyond ceil(n_rows / 8) is written (the 64-row words are stored bytewise), and out_bits may have any byte alignment.
 * pandrs_hip_predicate, col I64 or F64 (any other dtype: PANDRS_HIP_ERR_TYPE_MISMATCH).  The reference goes through
 * get_column_numeric_values, so every compare happens in f64: an I64 cell is first converted with (double)v (round to nearest
 * even, Rust's `as f64`), so 2^53 + 1 equals 2^53 under EQ, as in the reference.  With v the cell and a, b the arguments:
 *   GT / GE / LT / LE   !isnan(v) && v OP a
 *   EQ                  !isnan(v) && fabs(v - a) < DBL_EPSILON          NE   isnan(v) || fabs(v - a) >= DBL_EPSILON
 *                       (v = a = +inf: both false, inf - inf is NaN; the subtraction is rounded on its own, no fused operation)
 *   BETWEEN             a <= v && v <= b (between; is_between inclusive)          BETWEEN_EXCLUSIVE   a < v && v < b
 *   ISNA / NOTNA / IS_FINITE / IS_INFINITE   f64::is_nan / !is_nan / is_finite / is_infinite
 * A NaN a or b needs no special case: the expressions answer it.  b is read by the two BETWEEN ops only, a by neither of the last four.
 * pandrs_hip_isin: the reference compares to_bits() (functions.rs:152-155): -0.0 is not 0.0, and a NaN matches only a NaN with the
 * same payload.  The key compared, by the dtypes of col and values (any other pairing: PANDRS_HIP_ERR_TYPE_MISMATCH):
 *   F64 / F64          raw bits
 *   I64 / F64          the bits of (double)v, as in the reference
 *   I64 / I64          integers compared as integers (no reference counterpart: for ids beyond 2^53)
 *   U32CODE / U32CODE  string-pool codes (isin on a String column: the caller maps its strings to codes, unknown strings dropped)
 * values->null_mask must be NULL (PANDRS_HIP_ERR_INVALID_ARGUMENT); duplicates are allowed; n_values == 0 selects nothing (every
 * row with negate).  negate != 0 inverts every row's bit.
 * Deviation: a cell whose null bit is set behaves as NaN under pandrs_hip_predicate and never matches under pandrs_hip_isin (its
 * bit is 1 with negate); the cell under the bit is not looked at.  The reference fails on a missing value (src/dataframe/base.rs:
 * 555-561).  The same position as pandrs_hip_fill.
 * How (predicate.hip): rows in tiles, row p0 + r * 256 + tid, so every load is coalesced and one wave ballot is the 64-row word;
 * counts are popcounts summed per workgroup, one atomic add each.  Compare: one stream; for F64 the kernel is instantiated per op;
 * for I64, (double)v never decreases as v grows, so an op selects an interval of integers (NE: the complement of one) whose ends the
 * host finds by bisection with the very expression above, and the stream compares integers: the same bits, no conversion per row.
 * isin: an open-addressing set of 64-bit keys, a power-of-two slot count >= 2 x n_values, hashed with the library's key mixer
 * (integral f64 values differ in high bits only); the empty marker (all ones, also a NaN payload) is never stored: "the marker is
 * listed" is one flag.  Up to isin_lds_max_values = 4096 values every workgroup builds the set in LDS (at most 64 KiB of table + 64 bytes, two
 * workgroups per CU) with 64-bit compare-and-swap and probes it per row; beyond, one kernel builds it in the workspace and a second
 * probes it: the kernel boundary is the only hand-off, no workgroup waits for another, every insert and probe loop is bounded by the
 * slot count.  "isin_path" forces either; both give the same output.
 * Geometry (tests read it): predicate_tile_rows = 2048 rows per workgroup iteration, predicate_blocks_per_cu = 4, grid =
 * min(predicate_blocks_per_cu x compute units, ceil(n_rows / predicate_tile_rows)) workgroups striding over the tiles (an LDS set
 * beyond 32 KiB: 2 per compute unit).
 * Buffers: host columns, a host value list and a host out_bits are staged; device and resident columns are read in place.  Column
 * data and values are 8-byte aligned (4-byte for U32CODE); a null mask at any byte offset, bits past n_rows ignored.  mem_space,
 * values_mem_space and out_mem_space are independent.  out_count is a host pointer.  pandrs_hip_get_timings: the compare is
 * PANDRS_HIP_PHASE_AGGREGATE; isin's set is PANDRS_HIP_PHASE_BUILD, its stream PANDRS_HIP_PHASE_PROBE, table_slots the slot count,
 * n_partitions 1 for the LDS set and 2 for the global one.
 * Workspace, sized up front: the counter; for the global set 8 bytes per slot (16 to 32 bytes per listed value); staging: a host
 * column, a host value list and a host out_bits.  A memory_limit below either is PANDRS_HIP_ERR_OUT_OF_MEMORY.
 * Errors: ctx NULL: PANDRS_HIP_ERR_NOT_INITIALIZED; fewer rows than min_size_threshold: PANDRS_HIP_ERR_BELOW_THRESHOLD; a NULL col /
 * values, out_bits and out_count both NULL, an op outside 0 .. 11, n_rows < 0, n_values < 0, n_values > 2^30 or n_rows >= 2^32:
 * PANDRS_HIP_ERR_INVALID_ARGUMENT.  n_rows == 0: OK, nothing written, *out_count = 0.
 * Out of scope: combining two masks (and / or / not), predicates between two columns, string predicates (str_contains and the
 * like), where_cond / mask / clip, isin through the legacy string frame, the multi-GPU path. */
typedef enum pandrs_hip_pred_op {
    PANDRS_HIP_PRED_GT = 0, PANDRS_HIP_PRED_GE = 1, PANDRS_HIP_PRED_LT = 2, PANDRS_HIP_PRED_LE = 3,
    PANDRS_HIP_PRED_EQ = 4, PANDRS_HIP_PRED_NE = 5,
    PANDRS_HIP_PRED_BETWEEN = 6,            /* a <= v && v <= b */
    PANDRS_HIP_PRED_BETWEEN_EXCLUSIVE = 7,  /* a <  v && v <  b */
    PANDRS_HIP_PRED_ISNA = 8, PANDRS_HIP_PRED_NOTNA = 9, PANDRS_HIP_PRED_IS_FINITE = 10, PANDRS_HIP_PRED_IS_INFINITE = 11
} pandrs_hip_pred_op;

int32_t pandrs_hip_predicate(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows,
                             int32_t op, double a, double b, int32_t out_mem_space, uint8_t *out_bits, int64_t *out_count);

int32_t pandrs_hip_isin(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows,
                        int32_t values_mem_space, const pandrs_hip_column *values, int64_t n_values, int32_t negate,
                        int32_t out_mem_space, uint8_t *out_bits, int64_t *out_count);

/* ---- bins of one numeric column: cut, qcut, per-bin counts -----------------------------------------------------------------------
 * PandasCompatExt::value_range (src/dataframe/pandas_compat/functions.rs:2270-2282), cut (:2339-2368) and qcut (:2370-2420); the
 * reference's tests at :6840-6846 and :6943-7018.  Both read the column through get_column_numeric_values: every cell in f64, an
 * I64 cell as (double)v (so 2^53 + 1 falls where 2^53 falls).  With `valid` the cells that are not NaN and m their number:
 *   cut(bins)   w = (max - min) / bins as f64; e[i] = min + i as f64 * w for i = 0 ..= bins, then e[bins] = max + 0.001.
 *   qcut(q)     valid in ascending stable order; e[i] = valid[min((m as f64 * i as f64 / q as f64) as usize, m - 1)], i = 0 ..= q;
 *               when it looks a row up, the last edge is e[q] + 0.001.
 *   a row       NaN gives "NaN"; any other v the FIRST i in 0 .. bins with v >= e[i] && v < e[i + 1]; a row that matches no bin is
 *               left out of cut's result (it is shorter than the column: the maximum from about 2^43 upward, where max + 0.001 ==
 *               max) and is "" in qcut's.  The labels, "(lo, hi]" with {:.2} and "Q{i + 1}", are the mirrors' business.
 * pandrs_hip_bin_edges returns that edge list (without qcut's + 0.001, which the caller adds), pandrs_hip_bin takes any edge
 * list and answers per row: the code i, PANDRS_HIP_BIN_NONE (no bin) or PANDRS_HIP_BIN_NAN (a NaN cell), and the rows per code.
 * With a non-decreasing edge list the first match is i = (the number of edges <= v) - 1 wherever that lies in [0, n_bins):
 * e[i] <= v < e[i + 1] names i uniquely, and a bin with e[i] == e[i + 1] is empty either way; comparisons are by value (-0.0 ==
 * +0.0), +-inf edges are allowed, a NaN edge or a decreasing list is refused.  The reference's own lists never decrease except
 * where rounding leaves cut's e[bins] below e[bins - 1]; passing max(e[bins], e[bins - 1]) there selects the same rows, since no
 * row lies in [e[bins - 1], e[bins]) either way.  A non-finite w (an infinite min or max, max - min overflowing) makes e[0] NaN
 * and every bin empty: the caller answers that case from out_valid without a pandrs_hip_bin call.
 * Exactness: codes and counts are exact (comparisons and integers).  Every edge is bit for bit the reference's: min, max and the
 * selected elements are the column's own cells (I64: the selected integer as f64, also beyond 2^53), cut's expression is
 * evaluated on the host, every operation rounded on its own (no fused multiply-add).
 * Deviations:
 *  - a cell whose null bit is set behaves as NaN and the cell under the bit is not looked at (the reference fails on a missing
 *    value, src/dataframe/base.rs:555-561); it is not counted in out_valid.  The position of pandrs_hip_predicate and pandrs_hip_fill.
 *  - Signed zero: min, max and the selected elements come from the order-preserving code, -0.0 before +0.0 (pandrs_hip_describe),
 *    so an edge that is zero may differ from the reference's in its sign bit.  No code changes (comparisons are by value); a cut
 *    label may read "-0.00" for "0.00".
 *  - no valid cell: pandrs_hip_bin_edges is status OK with *out_valid = 0 and every edge NaN; the reference returns
 *    Err(InvalidValue) and the mirrors raise it, as for bins == 0 / q == 0.
 * How, pandrs_hip_bin (bin.hip): one stream over the column, 16-byte loads (two rows per thread and load; a data pointer 8 bytes
 * off a 16-byte boundary takes 8-byte loads), codes stored as coalesced int32 pairs: 8 bytes read and 4 written per row.  Every
 * workgroup copies the edges into LDS once ((bin_max_bins + 1) x 8 bytes = 32 KiB + 8 at most; the LDS is sized by n_bins).  Two
 * searches behind "bin_path": search, a branch-free upper bound of ceil(log2(n_bins + 1)) steps, the same for every lane; guess,
 * where the host finds e[0 .. n_bins) evenly spaced (n_bins >= 2, w = (e[n_bins - 1] - e[0]) / (n_bins - 1) finite and positive,
 * every |e[i] - (e[0] + i w)| <= w / 4; the last edge is free): (int)((v - e[0]) / w), clamped and corrected against the real
 * edges in LDS in at most 2 steps, a lane that is still off takes the search.  What a lane ends with satisfies e[i] <= v <
 * e[i + 1], so both give the same code for every row, also at an edge and one ulp off it.  "bin_path" 0 takes the guess from
 * bin_guess_min_bins = 128 evenly spaced bins on (measured: the search wins at 64 bins and loses at 256).  I64 cells are
 * converted per row.  Counts: a uint32 histogram of n_bins + 2 cells per workgroup in LDS; lanes of a wave that hold the same
 * code add once (up to 4 codes per wave and row by ballot, given up once a round folds fewer than 4 lanes; the rest by LDS
 * atomics), flushed with 64-bit atomics to workspace counters when the workgroup ends; out_counts == NULL compiles
 * the histogram out, out_codes == NULL leaves the histogram alone.  No workgroup waits for another; every row index is 64-bit.
 * How, pandrs_hip_bin_edges (describe.hip): CUT runs the moments stream of pandrs_hip_describe alone.  QCUT asks that file's
 * multi-rank radix select for integer ranks instead of percentiles, all weights zero; one selection takes up to 32 distinct
 * ranks, so k + 1 > 32 runs ceil((k + 1) / 32) selections over the column: correct, not fast.
 * Geometry (tests read it): bin_max_bins = 4096; bin_tile_rows = 2048 rows per workgroup iteration, bin_blocks_per_cu = 4, grid =
 * min(bin_blocks_per_cu x compute units, ceil(n_rows / bin_tile_rows)) workgroups striding over the tiles (with counts and more
 * than about 3400 bins the LDS leaves room for three workgroups per compute unit; the fourth follows).  pandrs_hip_bin_edges has
 * pandrs_hip_describe's geometry.
 * Buffers: a host column and a host out_codes are staged; device and resident columns are read in place.  Column data is 8-byte
 * aligned (16-byte alignment not needed); a null mask at any byte offset, bits past n_rows ignored.  out_codes receives exactly
 * n_rows int32 (4-byte aligned, no byte past 4 x n_rows written) and may be NULL; out_counts is a host pointer to n_bins + 2
 * int64, the bins, then NONE, then NAN, summing to n_rows, and may be NULL; not both.  edges, out_edges and out_valid are host
 * pointers.  pandrs_hip_get_timings: the stream is PANDRS_HIP_PHASE_AGGREGATE and n_partitions says which search ran (1 search,
 * 2 guess); pandrs_hip_bin_edges: PANDRS_HIP_PHASE_OTHER, n_partitions the number of selections.
 * Workspace, sized up front, whatever n_rows: pandrs_hip_bin the edges and the counters (12 bytes per bin); pandrs_hip_bin_edges
 * pandrs_hip_describe's.  Staging: a host column, a host out_codes.  A memory_limit below either is PANDRS_HIP_ERR_OUT_OF_MEMORY.
 * Errors: ctx NULL: PANDRS_HIP_ERR_NOT_INITIALIZED; fewer rows than min_size_threshold: PANDRS_HIP_ERR_BELOW_THRESHOLD; a column
 * that is not I64 / F64: PANDRS_HIP_ERR_TYPE_MISMATCH; a NULL col / edges / out_edges / out_valid, out_codes and out_counts both
 * NULL, n_bins or k outside 1 .. bin_max_bins, a kind outside the enum, an edge that is NaN or below the one before it, n_rows <
 * 0 or n_rows >= 2^32: PANDRS_HIP_ERR_INVALID_ARGUMENT.  pandrs_hip_bin with n_rows == 0: OK, nothing written to out_codes,
 * out_counts all zero.
 * Out of scope: more than 4096 bins; right-closed or labelled pandas-style intervals beyond the reference's strings; binning by a
 * second column's edges; String columns; a call between 2^31 and 2^32 rows as a tested size (the indexing is 64-bit by
 * construction); the multi-GPU path; fusing the codes into group_by without materialising them. */
#define PANDRS_HIP_BIN_MAX_BINS 4096
#define PANDRS_HIP_BIN_NONE (-1)        /* the row matches no bin */
#define PANDRS_HIP_BIN_NAN (-2)         /* the cell is NaN or null */
typedef enum pandrs_hip_bin_kind { PANDRS_HIP_BIN_CUT = 0, PANDRS_HIP_BIN_QCUT = 1 } pandrs_hip_bin_kind;

int32_t pandrs_hip_bin(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows, const double *edges,
                       int32_t n_bins, int32_t out_mem_space, int32_t *out_codes, int64_t *out_counts);

/* kind = pandrs_hip_bin_kind, k = bins (CUT) or q (QCUT); out_edges receives k + 1 doubles, *out_valid the cells that are
 * neither null nor NaN. */
int32_t pandrs_hip_bin_edges(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows, int32_t kind,
                             int32_t k, double *out_edges, int64_t *out_valid);

/* ---- distinct values of one column and their counts: value_counts, unique, nunique, mode, is_unique ------------------------------
 * PandasCompatExt::unique / value_counts (src/dataframe/pandas_compat/functions.rs:343-384), nunique (:775-788), value_counts_numeric /
 * unique_numeric (:1709-1753), mode_numeric / mode_string (:4120-4139) and mode_with_count / is_unique / nunique_all (:4226-4259).
 * Every one of them asks "which values does the column hold, and how often": pandrs_hip_distinct computes that list on the device
 * and keeps it in the context, pandrs_hip_distinct_fetch copies it out (two steps, as groupby_agg / groupby_fetch: the caller
 * allocates after it knows n_entries).
 * Entries: one per distinct number, then at most one NaN entry and one NULL entry.  An entry's value is an 8-byte cell as in
 * groupby_fetch (the i64, the f64 bits, a zero-extended code, 0 / 1), its flag 0 for a number, 1 for the NaN entry (value: the
 * canonical NaN 0x7FF8000000000000), 2 for the NULL entry (value 0).  All NaN payloads form one entry; -0.0 and 0.0 are two
 * entries (the reference keys on to_bits); a cell under a null bit is never looked at and nulls form the one NULL entry (the
 * engine's key rule, above: "a null key is its own group").  Counts are int64 and exact; they always sum to n_rows, and
 * n_valid + nan_count + null_count == n_rows.
 * Order: PANDRS_HIP_DISTINCT_BY_VALUE: numbers ascending in the total order of the order-preserving image of their bits (I64 as
 * signed integers; F64 -inf .. -0.0, 0.0 .. +inf, so -0.0 before 0.0; BOOLBITS false, true), then the NaN entry, then the NULL
 * entry.  U32CODE orders by code_rank[code] when code_rank (n_codes uint32, a permutation of 0 .. n_codes: the byte-wise string
 * order, as pandrs_hip_sort_indices takes it) is given and by code when it is NULL; with n_codes > 0 a code >= n_codes is
 * PANDRS_HIP_ERR_INVALID_ARGUMENT, found on the device with no fault, and the context serves the next call.
 * PANDRS_HIP_DISTINCT_BY_COUNT: count descending, ties in the value order above (functions.rs:366, :379-382).  Both orders are
 * fully determined: a result can be compared bit for bit.
 * max_count is the largest count among the numbers (0 if there is none) and n_modes how many numbers have it: under BY_COUNT
 * they need not be the first entries, since a NaN or NULL entry with a larger count comes before them.
 * Deviations: the reference keeps NaN payloads apart (one entry per payload; here one canonical entry); its order among values
 * that compare Equal under partial_cmp (NaNs, -0.0 / 0.0, equal counts) is HashMap order (here the total order above); it converts
 * I64 `as f64` before counting, so integers above 2^53 may merge (here they are counted as i64 and stay apart).
 * How (distinct.hip): a census stream (16-byte loads) finds min and max, the NaN / null / valid counts and for F64 whether every
 * number is integral with |v| <= 2^53 and whether a -0.0 is present.  Direct path (info.path 1): when the numbers span at most
 * distinct_direct_max_cells cells (max - min + 1 in unsigned 64-bit, so I64_MIN .. I64_MAX does not wrap; codes and bools by
 * value; F64 by (int64)v - min, only when all numbers are integral and no -0.0 is present) a second stream counts into a uint32
 * table in LDS: lanes of a wave holding the same cell add once by ballot, the rest by LDS atomics, so one hot value does not
 * serialise; a per-workgroup uint32 counter cannot overflow below 2^32 rows; non-zero cells are added to 64-bit workspace
 * counters when the workgroup ends, and one small kernel compacts them in ascending order.  8 bytes read per row and stream,
 * nothing written.  Engine path (info.path 2), everything else: the groupby engine with the column as the key and COUNT (its
 * doubles are exact below 2^53), its groups turned into entries on the device.  Both: the radix sort of pandrs_hip_sort_indices
 * orders the entries by (count descending,) class and order key, skipped where the direct table is already in order; a reduce
 * finds max_count and n_modes.  No workgroup waits for another; every row index is 64-bit.
 * Geometry (tests read it): distinct_direct_max_cells = 8192 (32 KiB of uint32 counters per 256-thread workgroup, four
 * workgroups per compute unit inside 160 KiB of LDS); distinct_tile_rows = 2048 rows per workgroup iteration;
 * distinct_blocks_per_cu = 4; grid = min(distinct_blocks_per_cu x compute units, ceil(n_rows / distinct_tile_rows)).
 * "distinct_path" (pandrs_hip_ctx_set_option): 0 = default and 1 = direct wherever it is possible, 2 = always the engine; the
 * same list either way.  pandrs_hip_get_timings: n_partitions reports the path taken (1 direct, 2 engine); the census is
 * PANDRS_HIP_PHASE_ESTIMATE, the direct stream PANDRS_HIP_PHASE_AGGREGATE.
 * Retained state: the list stays in the context until the next compute call on it, successful or not (every entry point that
 * starts a new pandrs_hip_get_timings record; the fetches, key_hash_cells and bytes_to_bitmap do not, and the list has an arena
 * of its own, so a fetch never serves bytes another call wrote); pandrs_hip_distinct_fetch without a list is
 * PANDRS_HIP_ERR_INVALID_ARGUMENT, may be repeated, and any of its pointers may be NULL.  A pandrs_hip_distinct call invalidates the retained groupby result (groupby_fetch / partials_split) on
 * both paths; the engine path also overwrites what pandrs_hip_groupby_agg overwrites: the join result (join_fetch / join_gather).
 * The grouping of pandrs_hip_groupby_indices, the filter selection and the shuffle buckets stay as they were.
 * Buffers: a host column and a host code_rank are staged; device and resident columns are read in place.  I64 / F64 data 8-byte
 * aligned (16 not needed), codes 4-byte aligned, a null mask at any byte offset, bits past n_rows ignored.  out_info is a host
 * pointer.  The fetch's outputs (in out_mem_space) receive n_entries cells / bytes / int64.
 * Workspace, sized up front: the census block and distinct_direct_max_cells counters whatever n_rows.  Sized at the stage that
 * needs them, since they depend on what the column holds: the entry lists (57 bytes per entry) once the entries are counted; on
 * the engine path groupby_agg's workspace, and for an order that is not skipped the sort's.  A memory_limit below any of them is
 * PANDRS_HIP_ERR_OUT_OF_MEMORY, which can therefore come after the census or the engine has run (nothing is retained then, and
 * the context serves the next call).  Every block is written before it is read.
 * Errors: ctx NULL: PANDRS_HIP_ERR_NOT_INITIALIZED; fewer rows than min_size_threshold: PANDRS_HIP_ERR_BELOW_THRESHOLD; a NULL col
 * / out_info, a CELL64 column or any other dtype outside I64 / F64 / U32CODE / BOOLBITS, an order outside the enum, code_rank
 * with another dtype or with n_codes == 0, n_codes < 0, n_rows < 0 or n_rows >= 2^32: PANDRS_HIP_ERR_INVALID_ARGUMENT.  n_rows ==
 * 0: OK, an empty list and all-zero info (a call like any other: it starts and ends a timings record).
 * Out of scope: a call between 2^31 and 2^32 rows is untested (the row arithmetic is 64-bit by construction); per-row codes
 * (to_categorical), duplicated / drop_duplicates; the multi-GPU path.  (crosstab is pandrs_hip_pivot, below.) */
typedef enum pandrs_hip_distinct_order { PANDRS_HIP_DISTINCT_BY_VALUE = 0, PANDRS_HIP_DISTINCT_BY_COUNT = 1 } pandrs_hip_distinct_order;

typedef struct pandrs_hip_distinct_info {
    int64_t n_entries;    /* entries of the retained list: distinct numbers, then at most one NaN entry and one NULL entry */
    int64_t n_valid;      /* rows that are neither null nor (F64) NaN */
    int64_t nan_count, null_count;
    int64_t max_count;    /* largest count among the non-NaN, non-NULL entries; 0 if none */
    int64_t n_modes;      /* how many such entries have it */
    int32_t path;         /* 1 = direct table, 2 = engine */
    int32_t reserved;
} pandrs_hip_distinct_info;

int32_t pandrs_hip_distinct(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows,
                            int32_t order, const uint32_t *code_rank, int64_t n_codes, pandrs_hip_distinct_info *out_info);
/* any pointer may be NULL */
int32_t pandrs_hip_distinct_fetch(pandrs_hip_ctx *ctx, int32_t out_mem_space, uint64_t *out_values, uint8_t *out_flags,
                                  int64_t *out_counts);

/* ---- a group-by over two key columns laid out as a dense matrix: crosstab, pivot_table, pivot / unstack ---------------------------
 * PandasCompatExt::crosstab (src/dataframe/pandas_compat/functions.rs:2138-2183), PivotTable with AggFunction Sum / Mean / Min / Max /
 * Count (src/pivot/mod.rs:12-250) and pivot / unstack (functions.rs:2471-2527).  The reference collects
 * HashMap<(String, String), Vec<f64>> with one string clone per row; here pandrs_hip_pivot computes the labels of either key column
 * and the R x C cells on the device and keeps them in the context, pandrs_hip_pivot_fetch copies them out (two steps, as distinct /
 * distinct_fetch: the caller allocates after it knows R and C).
 * Labels: key columns may be I64, F64, U32CODE (with an optional rank table) or BOOLBITS, with or without null masks.  The labels
 * of a column are its distinct numbers in pandrs_hip_distinct's BY_VALUE order (the order-preserving image of the bits: I64 as
 * signed integers; F64 -inf .. -0.0, 0.0 .. +inf, so -0.0 before 0.0; BOOLBITS false, true; U32CODE by rank[code] when the rank
 * table - n_codes uint32, a permutation: the byte-wise string order - is given, else by code), as 8-byte cells with flag 0; after
 * the numbers comes at most ONE missing label with flag 1 and cell 0: NaN cells and null cells of a key column form the same label
 * (the reference sees both as one string), and a cell under a null bit is never looked at.  With n_codes > 0 a code >= n_codes is
 * PANDRS_HIP_ERR_INVALID_ARGUMENT, found on the device with no fault, and the context serves the next call.
 * Cells: column-major, cell (index label i, columns label j) at [j * R + i]: the frame's output columns are per columns label.
 * out_rows[j * R + i] is the number of rows holding the pair, exact, as int64; 0 = the cell is absent; this is crosstab's answer,
 * and the rows sum to n_rows.  out_cells is NaN (0x7FF8000000000000) for an absent cell and otherwise what the groupby engine's
 * Sum / Mean / Min / Max / Count / Last (pandrs_hip_groupby_agg over the two key columns) gives for the group
 * (index label, columns label) of values_col, an I64 or F64 column with or without a mask: null value cells are skipped; Sum of
 * an I64 column wraps and is converted once; Mean divides by the non-null cells and is 0.0 when there is none; Min / Max skip NaN
 * cells, order -0.0 < 0.0, and answer 0.0 when no cell counts or the extreme is the sentinel (+inf / -inf, I64_MAX / I64_MIN);
 * Count is the rows of the cell, null and NaN value cells included; Last is the value at the cell's last row, 0.0 when it is
 * null.  PANDRS_HIP_PIVOT_ROWS (crosstab) takes no values column and out_cells holds the rows as doubles.
 * Min, Max, Count, Last and out_rows are bit for bit the engine's on both paths; Sum and Mean of F64 stay within the bound of the
 * device sums, 2 gamma_k sum|x| over the cell's own k rows, and are exact for I64 whose partial sums stay below 2^53.
 * Deviations (pivot/mod.rs:195-228, functions.rs:2492-2499, against the contract above): the reference's Count is values.len(), so it
 * counts NaN value cells, as here; its Min / Max are a fold from the first value with `if x < y` / `if x > y`, which keeps a
 * leading NaN and the earlier of -0.0 / 0.0 (here NaN cells are skipped and -0.0 < 0.0, as in the engine) and returns an extreme of
 * +inf / -inf as it is (here the engine's sentinel rule answers 0.0); its Sum / Mean fold in row order and divide by every row (here
 * within the bound above, null value cells skipped); an absent cell is the string "" in its legacy frame (here NaN, and the frame
 * masks it); its label order for pivot_table is HashSet order (here byte-wise ascending on the host, as in crosstab); pivot /
 * unstack insert into a HashMap per pair, so the last row of a pair wins: PANDRS_HIP_PIVOT_LAST, a null value cell as 0.0.
 * How (pivot.hip).  A census of both key columns (distinct.hpp, the census of pandrs_hip_distinct) gives min, max, the missing
 * counts, F64 integrality and -0.0 presence.  Direct path (info.path 1): both columns addressable by value under the rule of
 * distinct's direct path (codes and bools by value; I64 by v - min in unsigned 64-bit, so I64_MIN .. I64_MAX does not wrap; F64 by
 * (int64)v - min, only when all numbers are integral with |v| <= 2^53 and no -0.0 is present) and (span1 + 1) x (span2 + 1) <=
 * pivot_direct_max_cells, span = max - min + 1 value slots and the + 1 the missing slot.  ONE fused stream (16-byte loads where the
 * data is 16-byte aligned, 64-bit row arithmetic) reads the two keys and the value of each row and accumulates into a
 * per-workgroup table in LDS in span coordinates; there is no label lookup in the stream.  Lanes of a wave that hold the same
 * cell combine by ballot and a wave reduction before touching LDS, the rest use LDS atomics, so one hot cell does not
 * serialise; a per-workgroup uint32 counter cannot overflow below 2^32 rows; non-empty cells are folded into 64-bit / f64
 * workspace cells when the workgroup ends.  LAST keeps the largest row index per cell and the finish kernel gathers the value.
 * One small finish kernel drops span rows and span columns with no row (which yields the labels, ranked codes ordered by rank),
 * writes the dense R x C result and counts n_cells_present.  Key columns are read twice (census, stream), the value column once;
 * nothing per row is written.  General path (info.path 2), everything else: the groupby engine lists either column's distinct
 * cells (COUNT, as distinct's engine path) and the radix sort orders them into the label lists; R x C > pivot_max_cells answers
 * PANDRS_HIP_ERR_OPERATION_FAILED with out_info filled (labels, missing rows, path), nothing retained, and the context serves the
 * next call; the engine then runs with the two key columns, the op and COUNT, and a small kernel looks each GROUP's two key cells
 * up in the sorted label lists (a binary search over the order keys) and writes the group into its dense cell; cells no group
 * reached stay absent.  An F64 key column holding NaN cells gets a bit mask with the NaN cells added (n_rows / 8 bytes), so that
 * the engine meets one missing group.  No per-row code column is materialised on either path; no workgroup waits for another.
 * Geometry (tests read it): pivot_direct_max_cells = 4096 table cells, the missing slots included (LDS bytes per 256-thread
 * workgroup: 4 per cell for ROWS / COUNT, 12 for MIN / MAX / LAST, 16 for SUM / MEAN, so at most 64 KiB: two to four
 * workgroups per compute unit inside 160 KiB of LDS, more for small tables); pivot_max_cells = 16777216 (16 bytes per retained
 * cell: the dense result stays at 256 MiB); pivot_tile_rows = 2048 rows per workgroup iteration; pivot_blocks_per_cu = 4;
 * grid = min(pivot_blocks_per_cu x compute units, ceil(n_rows / pivot_tile_rows)).
 * "pivot_path" (pandrs_hip_ctx_set_option): 0 = default and 1 = direct wherever it is possible, 2 = always the general path; the
 * same result either way.  pandrs_hip_get_timings: n_partitions reports the path taken (1 direct, 2 general); the census is
 * PANDRS_HIP_PHASE_ESTIMATE, the direct stream PANDRS_HIP_PHASE_AGGREGATE.
 * Retained state: the result stays in the context, in an arena of its own, until the next compute call on it, successful or not
 * (as the distinct list); pandrs_hip_pivot_fetch without a result is PANDRS_HIP_ERR_INVALID_ARGUMENT, may be repeated, and any of
 * its pointers may be NULL.  A pandrs_hip_pivot call invalidates the retained groupby result (groupby_fetch / partials_split) and
 * the distinct list on both paths; the general path also overwrites what pandrs_hip_groupby_agg overwrites: the join result
 * (join_fetch / join_gather).  The grouping of pandrs_hip_groupby_indices, the filter selection and the shuffle buckets stay.
 * Buffers: host columns and host rank tables are staged; device and resident columns are read in place.  I64 / F64 data 8-byte
 * aligned (16 not needed), codes 4-byte aligned, null masks at any byte offset, bits past n_rows ignored.  out_info is a host
 * pointer.  The fetch's outputs (in out_mem_space) receive R / C labels and flags and R x C cells / rows.
 * Workspace, sized up front: the two census blocks and three pivot_direct_max_cells tables whatever n_rows; on the direct path
 * the result for the span table (at most pivot_direct_max_cells cells).  Sized at the stage that needs them: on the general path
 * the NaN masks after the census, either label list (41 bytes per label) once the engine has counted the column's cells,
 * groupby_agg's and the sort's workspace, and the dense result (16 bytes per cell, 9 per label) once R and C are known.  A
 * memory_limit below any of them is PANDRS_HIP_ERR_OUT_OF_MEMORY, which can therefore come after the census or an engine run
 * (nothing is retained then, and the context serves the next call).  Every block is written before it is read.
 * Errors: ctx NULL: PANDRS_HIP_ERR_NOT_INITIALIZED; fewer rows than min_size_threshold: PANDRS_HIP_ERR_BELOW_THRESHOLD; a NULL
 * index_col / columns_col / out_info, a values column given with PANDRS_HIP_PIVOT_ROWS or missing otherwise, a key dtype outside
 * I64 / F64 / U32CODE / BOOLBITS (CELL64 included), a values dtype outside I64 / F64, an op outside the enum, a rank table with
 * another dtype or with n_codes == 0, n_codes < 0, n_rows < 0 or n_rows >= 2^32: PANDRS_HIP_ERR_INVALID_ARGUMENT.  n_rows == 0: OK,
 * an empty result (R = C = 0) and all-zero info (a call like any other: it starts and ends a timings record).
 * Out of scope: to_categorical (its first-appearance codes need another pass); duplicated / drop_duplicates; more than one
 * index, columns or values column; margins; the legacy string frame; the multi-GPU path; a call between 2^31 and 2^32 rows is
 * untested (the row arithmetic is 64-bit by construction). */
typedef enum pandrs_hip_pivot_op {
    PANDRS_HIP_PIVOT_ROWS = 0,   /* crosstab: rows per cell, values_col must be NULL */
    PANDRS_HIP_PIVOT_SUM = 1,
    PANDRS_HIP_PIVOT_MEAN = 2,
    PANDRS_HIP_PIVOT_MIN = 3,
    PANDRS_HIP_PIVOT_MAX = 4,
    PANDRS_HIP_PIVOT_COUNT = 5,  /* the five of pivot/mod.rs:12-23 */
    PANDRS_HIP_PIVOT_LAST = 6    /* pivot / unstack: the last row of the pair wins */
} pandrs_hip_pivot_op;

typedef struct pandrs_hip_pivot_info {
    int64_t n_index_labels, n_column_labels;   /* R, C */
    int64_t n_cells_present;                   /* cells with at least one row */
    int64_t index_missing_rows, column_missing_rows;   /* rows whose index / columns cell is NaN or null */
    int32_t path;                              /* 1 = direct, 2 = general */
    int32_t reserved;
} pandrs_hip_pivot_info;

int32_t pandrs_hip_pivot(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *index_col, const uint32_t *index_rank,
                         int64_t n_index_codes, const pandrs_hip_column *columns_col, const uint32_t *columns_rank,
                         int64_t n_columns_codes, const pandrs_hip_column *values_col, int64_t n_rows, int32_t op,
                         pandrs_hip_pivot_info *out_info);
/* any pointer may be NULL */
int32_t pandrs_hip_pivot_fetch(pandrs_hip_ctx *ctx, int32_t out_mem_space, uint64_t *out_index_labels, uint8_t *out_index_flags,
                               uint64_t *out_column_labels, uint8_t *out_column_flags, double *out_cells, int64_t *out_rows);

/* ---- running folds and lagged differences of one numeric column: cumsum, cumprod, cummax, cummin, cumcount, shift, diff ------
 * PandasCompatExt::cumsum / cumprod / cummax / cummin (src/dataframe/pandas_compat/functions.rs:280-327), shift (:328-342),
 * pct_change (:514-530), diff (:531-541), cumcount (:2081-2094); known answers :4411-4447, :4547-4573, :6580-6595.  One column,
 * I64 or F64, with or without a null mask; an I64 cell is read `as f64`, as the reference's get_column_numeric_values does.  The
 * output is F64 for every op except CUM_COUNT, which writes I64.  A NaN this library produces is the canonical quiet NaN
 * 0x7FF8000000000000.
 * pandrs_hip_cumulative: row i covers rows 0 .. i.
 *   SUM    the reference's fold from +0.0: a column of only -0.0 gives +0.0, a NaN cell makes every later row NaN, +-inf behave
 *          as IEEE.  A parallel sum rounds differently from the sequential one: with u = 2^-53, gamma_k = k u / (1 - k u) and k
 *          the non-null rows in 0 .. i, wherever the running sum of |x| stays finite |got_i - ref_i| <= 2 gamma_k sum_{j<=i}|x_j|
 *          (both folds are within gamma_k sum|x| of the true sum).  Integer-valued inputs whose sum|x| stays below 2^53: bit for
 *          bit.  The state is a plain f64.
 *   PROD   the reference's fold from 1.0.  A workgroup-local product of ordinary data leaves f64's range where no running product
 *          does ([1e-200, 1e200, 1e200, 1e-200]), so the state is a mantissa and an integer exponent (frexp / ldexp); 0, +-inf
 *          and NaN stay in the mantissa, where IEEE multiplication gives the reference's class and sign.  Wherever every
 *          reference running product up to row i is normal, zero by a zero input, infinite by an infinite input, or NaN, the
 *          relative error is at most 2 gamma_k and class and sign are exact.  The reference is sticky after a range excursion of
 *          finite nonzero inputs (an overflow stays +-inf, an underflow to zero stays +-0, a later 0 or inf turns them into NaN):
 *          the apply pass records the first row r whose extended-range product converts to +-inf or 0, and the rows after r are
 *          rewritten by one more scan that starts at r + 1 from that converted value (0 and inf absorb: no second detection).
 *   MAX / MIN  f64::max / f64::min folds from -inf / +inf, bit for bit.  A NaN cell is skipped and outputs the running value
 *          (-inf / +inf before the first number).  Signed zeros as pandrs_hip_window's min / max: -0.0 is below +0.0.
 *   COUNT  the rows in 0 .. i that are neither null nor NaN, exact, as I64.
 * pandrs_hip_lag: every result bit for bit, every operation rounded on its own (no fused multiply-add).
 *   SHIFT       out[i] = x[i - periods], any sign of periods.  A row with no source is the reference's None, and one whose
 *               source is null is treated the same: NaN with its bit set.  |periods| >= n_rows leaves every row missing.
 *   DIFF        rows i < periods are NaN values with bit 0 (the reference's vec![NAN; n]); every other row x[i] - x[i - periods].
 *               periods = 0 is valid and computes x - x.
 *   PCT_CHANGE  rows i < periods as DIFF; elsewhere prev == 0.0 (and -0.0) gives NaN, otherwise (curr - prev) / prev.
 *   For DIFF and PCT_CHANGE a row with a null operand is NaN with its bit set; periods < 0: PANDRS_HIP_ERR_INVALID_ARGUMENT.
 * Deviations:
 *  - the reference has no null mask on these paths.  Here a row under a null bit is skipped: it outputs NaN, its bit is set in
 *    out_null_mask and the running value passes through unchanged; CUM_COUNT writes the running count there and sets no bit.
 *  - a running product that passes through a subnormal value keeps here the bits the reference loses.
 *  - a NaN cell that SHIFT copies arrives as the canonical NaN, whatever its payload.
 * How (cumulative.hip): reduce then apply over contiguous spans.  The column is cut into tiles of cum_tile_rows rows and each of
 * the grid's workgroups owns a contiguous span of whole tiles.  Kernel 1 folds every span into one summary; the prologue of
 * kernel 2 folds the summaries of the spans before its own (at most grid states, read from L2: no third kernel, no
 * single-workgroup pass that grows with n_rows), then scans its tiles from that carry and writes: two reads and one write of the
 * column.  Every hand-off between workgroups is a kernel boundary; no workgroup waits for another.  A lane loads and stores two
 * consecutive cells as 16 bytes (two 8-byte accesses when the buffer is only 8-byte aligned), a wave 128 consecutive rows per
 * instruction, four loads in flight; the scan runs in that order: the lane's pair, a wave scan by cross-lane moves, the loads
 * chained, the waves through LDS with one barrier per tile.  PROD launches the pair twice; the second ends at once when no row
 * left f64's range.  Lag is one stream: a row reads x[i] and x[i - periods].
 * Geometry (tests read it): cum_tile_rows = 2048 rows, cum_blocks_per_cu = 4, grid = min(cum_blocks_per_cu x compute units,
 * ceil(n_rows / cum_tile_rows)) workgroups; span b holds tiles / grid tiles and one more when b < tiles % grid.
 * Buffers: col is I64 or F64; any other dtype: PANDRS_HIP_ERR_TYPE_MISMATCH.  Host columns and outputs are staged; device and
 * resident columns are read in place.  Data and out_data are 8-byte aligned (16 is not required); the masks may sit at any byte
 * offset, input bits past n_rows are ignored.  out_data receives n_rows x 8 bytes.  out_null_mask receives exactly
 * ceil(n_rows / 8) bytes, bits past n_rows in the last byte 0, and no byte beyond is touched (stored bytewise); it may be NULL.
 * out_data or out_null_mask overlapping the column's data or mask in the same memory space: PANDRS_HIP_ERR_INVALID_ARGUMENT (the
 * column is read twice, so the call cannot run in place).  out_n_null is a host pointer and may be NULL: the bits set.
 * pandrs_hip_get_timings: the phase is PANDRS_HIP_PHASE_AGGREGATE, n_partitions is 0, algorithmic_bytes counts the streams run.
 * Workspace, sized up front in one arena: one 16-byte summary per workgroup of the full grid, the excursion cell and the counter
 * (lag: the counter only); staging: a host column and host outputs.  A memory_limit below either is PANDRS_HIP_ERR_OUT_OF_MEMORY.
 * Errors: ctx NULL: PANDRS_HIP_ERR_NOT_INITIALIZED; fewer rows than min_size_threshold: PANDRS_HIP_ERR_BELOW_THRESHOLD; a NULL
 * col / out_data, an op outside its enum, n_rows < 0 or n_rows >= 2^32: PANDRS_HIP_ERR_INVALID_ARGUMENT.  n_rows == 0: OK,
 * nothing written, *out_n_null = 0.
 * Out of scope: clip, skipna= and reverse scans, String and Boolean columns, the legacy string frame,
 * TimeSeries::{diff,shift,pct_change}.  The group-wise cumulative ops are pandrs_hip_grouped, below. */
typedef enum pandrs_hip_cum_op {
    PANDRS_HIP_CUM_SUM = 0, PANDRS_HIP_CUM_PROD = 1, PANDRS_HIP_CUM_MAX = 2, PANDRS_HIP_CUM_MIN = 3, PANDRS_HIP_CUM_COUNT = 4
} pandrs_hip_cum_op;

typedef enum pandrs_hip_lag_op {
    PANDRS_HIP_LAG_SHIFT = 0, PANDRS_HIP_LAG_DIFF = 1, PANDRS_HIP_LAG_PCT_CHANGE = 2
} pandrs_hip_lag_op;

int32_t pandrs_hip_cumulative(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows,
                              int32_t op, int32_t out_mem_space, void *out_data, uint8_t *out_null_mask, int64_t *out_n_null);

int32_t pandrs_hip_lag(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows, int32_t op,
                       int64_t periods, int32_t out_mem_space, void *out_data, uint8_t *out_null_mask, int64_t *out_n_null);

/* ---- the same folds and lags within groups: GroupBy cumsum, cummax, cummin, cumcount, row_number, shift, diff, pct_change ------------
 * The reference's GroupWise*Ops (src/dataframe/groupby_window.rs) are marked "simplified implementation" and ignore the group
 * columns, so the semantics are this header's own: a grouped op gives, for every group, the result of the ungrouped op on that
 * group's rows in ascending row order, written back at those rows' positions.
 * Which groups: the ones the context retains from its last successful pandrs_hip_groupby_indices (rows, offsets, n_groups,
 * n_rows).  One grouping serves any number of grouped calls; the keys are whatever that call took (any dtype, several keys, NULL
 * keys as one group per distinct combination).  No retained grouping, or n_rows different from the grouping's:
 * PANDRS_HIP_ERR_INVALID_ARGUMENT, and the message says which.  A grouped call takes its scratch from the work arena and leaves
 * the retained grouping as it was.
 * Within group g, with rows r_0 < r_1 < ..., row r_t answers:
 *   CUM_SUM / CUM_MAX / CUM_MIN / CUM_COUNT   pandrs_hip_cumulative's contract over r_0 .. r_t.  SUM folds from +0.0 (a group of
 *          only -0.0 gives +0.0; a NaN or +-inf cell affects later rows of its own group only).  MAX / MIN fold from -inf /
 *          +inf, skip NaN cells, hold -0.0 below +0.0, bit for bit.  COUNT is I64: the rows so far in the group that are neither
 *          null nor NaN.  A row under a null bit answers NaN with its output bit set and the running value passes through; COUNT
 *          writes the running count there and sets no bit.  SUM's accuracy: |got - ref| <= 2 gamma_k sum|x|, k and the sum over
 *          the group's own prefix, wherever that running sum of |x| stays finite; integer-valued data with sum|x| below 2^53 per
 *          group: bit for bit.  A group's prefix is folded from its own cells only: it is never a global prefix minus the prefix
 *          at the group's start, which would cancel across groups.
 *   ROW_NUMBER   I64, the value t.  Every row counts, null or not; col may be NULL and is not read; no null bit is set.
 *   SHIFT / DIFF / PCT_CHANGE   pandrs_hip_lag's contract with "row i - periods" read as r_{t - periods} of the same group; a
 *          source position outside the group is treated like a source row before row 0.  SHIFT takes either sign of periods;
 *          DIFF / PCT_CHANGE with periods < 0: PANDRS_HIP_ERR_INVALID_ARGUMENT.  Bit for bit, every operation rounded on its own
 *          (no fused multiply-add); a NaN that SHIFT copies arrives canonical (0x7FF8000000000000).
 * The output is F64 for every op except CUM_COUNT and ROW_NUMBER, which write I64.  periods is read by the three lag ops only.
 * How (grouped.hip): the work runs in sorted-position order (position j holds row rows[j]; a group is the contiguous positions
 * offsets[g] .. offsets[g + 1]).  Group heads are bit words, one bit per position, set from offsets by atomic ORs (one per word and wave).
 * The folds are a segmented reduce-then-apply over contiguous spans of whole tiles, the operator on (head seen, value) pairs:
 * kernel 1 gathers the column through rows[] once, leaves the cells and their null bits (as ballot words) contiguous in the
 * workspace and folds each span into a summary (does it hold a head; the fold of the cells after its last head); the prologue of
 * kernel 2 folds the summaries of earlier spans back to the nearest span that holds a head, then scans its tiles with a
 * cross-lane scan driven by the head word and scatters out[rows[j]].  Lag and ROW_NUMBER take the group's first position per
 * position from one ordinary max-scan of the head positions (the same tile scan) into a 32-bit array; j' = j - periods is in
 * the group iff 0 <= j' < n_rows and start[j'] == start[j]; lag reads the gathered cells, so the column is gathered once there
 * too.  Every hand-off between workgroups is a kernel boundary; no workgroup waits for another; no kernel uses scratch.
 * The output mask of a fold is the input mask with the bits past n_rows cleared (a copy, no scatter), all zero for COUNT and
 * ROW_NUMBER; lag builds it in a zeroed, aligned workspace bitmap with atomic ORs on 32-bit words and stores it bytewise.
 * Geometry (tests read it): grouped_tile_rows = 2048 positions, grouped_blocks_per_cu = 4, grid = min(grouped_blocks_per_cu x
 * compute units, ceil(n_rows / grouped_tile_rows)) workgroups; span b holds tiles / grid tiles and one more when b < tiles % grid.
 * Buffers and errors as pandrs_hip_cumulative: col is I64 or F64, any other dtype PANDRS_HIP_ERR_TYPE_MISMATCH; host columns and
 * outputs are staged, device and resident columns are read in place; data and out_data are 8-byte aligned, the masks may sit at
 * any byte offset, input bits past n_rows are ignored; out_null_mask receives exactly ceil(n_rows / 8) bytes stored bytewise, no
 * byte beyond touched, and may be NULL; an output overlapping the column in the same memory space:
 * PANDRS_HIP_ERR_INVALID_ARGUMENT; out_n_null is a host pointer and may be NULL.  n_rows == 0 (with a retained grouping of 0
 * rows): OK, nothing written.  ctx NULL: PANDRS_HIP_ERR_NOT_INITIALIZED; fewer rows than min_size_threshold:
 * PANDRS_HIP_ERR_BELOW_THRESHOLD; an op outside the enum: PANDRS_HIP_ERR_INVALID_ARGUMENT.  The row limit is the grouping's:
 * fewer than 2^32 - 16384 rows.
 * Workspace, sized up front in one arena, in bytes per row: 8 for the gathered cells (not ROW_NUMBER), 4 for the group starts
 * (lag and ROW_NUMBER), 2/8 for the head and null words, 1/8 for the lag bitmap; plus 12 bytes per workgroup of the full grid and
 * the counter.  Staging: a host column and host outputs.  A memory_limit below either is PANDRS_HIP_ERR_OUT_OF_MEMORY.
 * pandrs_hip_get_timings: the phase is PANDRS_HIP_PHASE_AGGREGATE, n_partitions is 0, algorithmic_bytes counts the streams run.
 * Out of scope: a grouped PROD (the sticky range-excursion rewrite of pandrs_hip_cumulative has no obvious per-group form),
 * group-wise fills, a grouped rank, a grouped top-k and group-wise windows, String and Boolean columns. */
typedef enum pandrs_hip_grouped_op {
    PANDRS_HIP_GROUPED_CUM_SUM = 0, PANDRS_HIP_GROUPED_CUM_MAX = 1, PANDRS_HIP_GROUPED_CUM_MIN = 2,
    PANDRS_HIP_GROUPED_CUM_COUNT = 3, PANDRS_HIP_GROUPED_ROW_NUMBER = 4,
    PANDRS_HIP_GROUPED_SHIFT = 5, PANDRS_HIP_GROUPED_DIFF = 6, PANDRS_HIP_GROUPED_PCT_CHANGE = 7
} pandrs_hip_grouped_op;

int32_t pandrs_hip_grouped(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows, int32_t op,
                           int64_t periods, int32_t out_mem_space, void *out_data, uint8_t *out_null_mask, int64_t *out_n_null);

/* ---- derived columns: one postfix program over up to eight columns, evaluated per row in one stream -----------------------------
 * What the predicate and cumulative blocks above leave out (combining masks, predicates between two columns, where_cond / mask /
 * clip) is pandrs_hip_eval.  PandasCompatExt::add_scalar / sub_scalar / mul_scalar / div_scalar / sqrt
 * (src/dataframe/pandas_compat/functions.rs:2819-2840), col_add / col_sub / col_mul / col_div (:2851-2960), add_columns .. div_columns
 * (:3890-3984), coalesce (:3846), clip (:237), where_cond / mask (:1079-1139), sign (:3998-4014), normalize (:2316-2337), and neg /
 * floor / ceil / trunc / fract / reciprocal / abs_column / round_column / mod_column / floordiv (helpers/math_ops.rs) are one program
 * each, and so is any expression over them: a * b + c > 0 costs its algorithmic bytes once, not one read and one write per operator.
 * The program is postfix over a typed stack of values (f64) and booleans: ops[i] is a pandrs_hip_eval_op, args[i] is read by COL
 * (a column index, integral, in [0, n_cols)) and CONST (the constant) and ignored by the rest.  Every operation is the reference's
 * Rust expression, rounded on its own (no fused multiply-add):
 *   COL        an I64 cell pushes (double)v (Rust's `as f64`: 2^53 + 1 loads as 2^53, as in pandrs_hip_predicate), an F64 cell its
 *              value, a BOOLBITS cell a boolean.  A numeric cell under a null bit loads as NaN, a boolean one as false; the cell
 *              under the bit is not read (the position of pandrs_hip_predicate and pandrs_hip_fill).  Any other dtype:
 *              PANDRS_HIP_ERR_TYPE_MISMATCH.
 *   CONST      pushes args[i], any f64.
 *   ADD SUB MUL DIV   IEEE.          REM   C fmod, Rust's %.
 *   MAX MIN    f64::max / f64::min: a NaN operand is ignored, NaN only from two NaNs; of +0.0 and -0.0 either may result.
 *   NEG ABS FLOOR CEIL TRUNC   exact.    ROUND   half away from zero (f64::round).    FRACT   x - trunc(x).
 *   SQRT       correctly rounded.        SIGN    1.0 / -1.0, and +0.0 for both zeros and NaN (functions.rs:3998-4014).
 *   GT GE LT LE EQ NE   the IEEE compares of two values -> a boolean (NOT the EPSILON compare of eq_value: that is PRED_EQ).
 *   ISNAN ISINF ISFINITE   a value -> a boolean.        AND OR NOT   booleans.
 *   SELECT     pops b, a, cond (cond pushed first) and pushes cond ? a : b; a and b have the same type.
 * Limits: 1 <= n_ops <= 64, 1 <= n_cols <= 8, at most 8 entries on the stack, exactly one entry left at the end, n_rows < 2^32.
 * Output of a value program: out_data receives n_rows doubles; every NaN result is stored as 0x7FF8000000000000, so all output
 * bits are defined.  The output null bit is set exactly where the result is NaN AND a cell of a column the program names was null
 * in that row (whichever branch a SELECT took).  out_null_mask receives exactly ceil(n_rows / 8) bytes, bits past n_rows 0, no
 * byte beyond touched; it may be NULL, and *out_count (a host pointer, may be NULL) is the number of such bits either way.
 * Output of a boolean program: out_data is the bitmap with pandrs_hip_predicate's conventions: LSB-first, bit = 1 the row is
 * selected, ceil(n_rows / 8) bytes stored bytewise, zero tail bits, any byte alignment: the data of a BOOLBITS column, which
 * pandrs_hip_filter_indices takes in place.  out_null_mask must be NULL.  out_data may be NULL (the count only) when out_count is
 * not; *out_count = the number of set bits.
 * An output overlapping the data or the mask of a named column in the same memory space: PANDRS_HIP_ERR_INVALID_ARGUMENT (as
 * pandrs_hip_lag, the call does not run in place).
 * pandrs_hip_eval_check is the same validator with no context and no device: col_dtypes[j] is the dtype of column j;
 * *out_is_mask = 1 for a boolean program, *out_depth = the deepest the stack gets (either may be NULL).
 * How (eval.hip): where every entry of a postfix program sits on the stack is known before it runs, so the host lowers the program
 * to three-address code (op, slot) and passes it by value in the kernel arguments: the dispatch is scalar and uniform, the eight
 * slots are named registers picked by a uniform switch, nothing is indexed at run time and no kernel uses scratch.  One stream:
 * a wave owns 128 consecutive rows per step, a lane two consecutive rows (16-byte loads and stores of 8-byte cells, two 8-byte
 * accesses when the buffer is only 8-byte aligned); every distinct named column is loaded once per row, the result leaves with
 * one store.  Bits leave as two wave ballots woven into the 128-row word; the count is one atomic add per workgroup.  Kernel
 * boundaries are the only hand-off.
 * Geometry (tests read it): eval_tile_rows = 2048 rows per workgroup iteration, eval_blocks_per_cu = 4, grid =
 * min(eval_blocks_per_cu x compute units, ceil(n_rows / eval_tile_rows)) workgroups striding over the tiles.
 * Buffers: the named host columns and host outputs are staged; device and resident columns are read in place; a column no COL
 * names is not looked at.  I64 / F64 data and a value out_data are 8-byte aligned (16 is not required); BOOLBITS data, the masks
 * and a bitmap may sit at any byte offset, input bits past n_rows are ignored.  pandrs_hip_get_timings: the phase is
 * PANDRS_HIP_PHASE_AGGREGATE, algorithmic_bytes counts every named column and the outputs once.
 * Workspace, sized up front: the counter; staging: the named host columns and host outputs.  A memory_limit below either is
 * PANDRS_HIP_ERR_OUT_OF_MEMORY.
 * Errors: ctx NULL: PANDRS_HIP_ERR_NOT_INITIALIZED (checked first); fewer rows than min_size_threshold:
 * PANDRS_HIP_ERR_BELOW_THRESHOLD; stack underflow, an operand of the wrong type, more than one entry left, a ninth entry, an op
 * outside 0 .. 30, a column index that is not an integer in [0, n_cols), n_ops or n_cols outside their limits, a NULL cols / ops /
 * args, no output, n_rows < 0 or n_rows >= 2^32: PANDRS_HIP_ERR_INVALID_ARGUMENT, and pandrs_hip_last_error names the op index
 * ("op 3: ...").  n_rows == 0: OK after the program is checked, nothing written, *out_count = 0.
 * Out of scope: pow / log / exp (the device's libm is not glibc's), replace_numeric (a value table is pandrs_hip_isin's set),
 * zscore, string ops and the legacy query strings, group-wise variants, the multi-GPU path. */
typedef enum pandrs_hip_eval_op {
    PANDRS_HIP_EVAL_COL = 0, PANDRS_HIP_EVAL_CONST = 1,
    PANDRS_HIP_EVAL_ADD = 2, PANDRS_HIP_EVAL_SUB = 3, PANDRS_HIP_EVAL_MUL = 4, PANDRS_HIP_EVAL_DIV = 5, PANDRS_HIP_EVAL_REM = 6,
    PANDRS_HIP_EVAL_MAX = 7, PANDRS_HIP_EVAL_MIN = 8,
    PANDRS_HIP_EVAL_NEG = 9, PANDRS_HIP_EVAL_ABS = 10, PANDRS_HIP_EVAL_FLOOR = 11, PANDRS_HIP_EVAL_CEIL = 12, PANDRS_HIP_EVAL_TRUNC = 13,
    PANDRS_HIP_EVAL_ROUND = 14, PANDRS_HIP_EVAL_FRACT = 15, PANDRS_HIP_EVAL_SQRT = 16, PANDRS_HIP_EVAL_SIGN = 17,
    PANDRS_HIP_EVAL_GT = 18, PANDRS_HIP_EVAL_GE = 19, PANDRS_HIP_EVAL_LT = 20, PANDRS_HIP_EVAL_LE = 21, PANDRS_HIP_EVAL_EQ = 22,
    PANDRS_HIP_EVAL_NE = 23,
    PANDRS_HIP_EVAL_ISNAN = 24, PANDRS_HIP_EVAL_ISINF = 25, PANDRS_HIP_EVAL_ISFINITE = 26,
    PANDRS_HIP_EVAL_AND = 27, PANDRS_HIP_EVAL_OR = 28, PANDRS_HIP_EVAL_NOT = 29,
    PANDRS_HIP_EVAL_SELECT = 30             /* pops b, a, cond: cond ? a : b */
} pandrs_hip_eval_op;

int32_t pandrs_hip_eval(pandrs_hip_ctx *ctx, int32_t mem_space, const pandrs_hip_column *cols, int32_t n_cols,
                        int64_t n_rows, const int32_t *ops, const double *args, int32_t n_ops,
                        int32_t out_mem_space, void *out_data, uint8_t *out_null_mask, int64_t *out_count);

int32_t pandrs_hip_eval_check(const int32_t *col_dtypes, int32_t n_cols, const int32_t *ops, const double *args,
                              int32_t n_ops, int32_t *out_is_mask, int32_t *out_depth);

/* ---- whole-column reductions ----------------------------------------------
 * Replaces simd_{sum,mean,min,max}_{f64,i64} (src/optimized/jit/simd.rs:9-112) and
 * Int64Column/Float64Column::{sum,mean,min,max}.  out[0..3] = sum, mean, min, max as f64;
 * out_count = number of non-null elements.  Empty input: sum 0, mean 0 (simd.rs), min/max
 * +inf/-inf for f64 and i64::MAX/MIN (as f64) for i64. */
int32_t pandrs_hip_reduce_column(pandrs_hip_ctx *ctx, int32_t mem_space,
                                 const pandrs_hip_column *col, int64_t n,
                                 double out[4], int64_t *out_count);

/* (sum, sum of squares, count) of the non-null values as f64 — the accumulator triple of
 * parallel_std_f64 / parallel_var_f64 (src/optimized/jit/parallel.rs:190-250), from which the caller
 * derives the reference's POPULATION variance  max(sum_sq / n - mean^2, 0)  (:222-233; n <= 1 => 0). */
int32_t pandrs_hip_reduce_moments(pandrs_hip_ctx *ctx, int32_t mem_space,
                                  const pandrs_hip_column *col, int64_t n,
                                  double *out_sum, double *out_sum_sq, int64_t *out_count);

/* ---- multi-GPU: the exchange inside the library (no reference counterpart: ---------------------
 * src/gpu/multi_gpu.rs:326-360 splits rows on the host, src/distributed is an in-process DataFusion wrapper).
 * One process per GPU; every rank calls the same entry point with its own row-range shard.  RCCL is opened at run
 * time (librccl.so.1), so single-GPU users do not need it.
 *
 * pandrs_hip_comm wraps an ncclComm_t: rank 0 calls comm_unique_id, the host distributes the 128 bytes (any
 * channel), every rank calls comm_init; or comm_adopt takes an ncclComm_t the host already owns. */
typedef struct pandrs_hip_comm pandrs_hip_comm;
int32_t pandrs_hip_comm_unique_id(char out_id[128]);
int32_t pandrs_hip_comm_init(pandrs_hip_ctx *ctx, const char id[128], int32_t rank, int32_t world, pandrs_hip_comm **out_comm);
int32_t pandrs_hip_comm_adopt(void *nccl_comm, int32_t rank, int32_t world, pandrs_hip_comm **out_comm);
/* Any other fabric (and the multi-rank tests on one GPU): the collectives the exchange needs, as host callbacks over
 * HOST buffers — the library stages its device buffers through them.  Every callback returns 0 on success and is
 * called by every rank in the same order:
 *   all_gather          every rank contributes `bytes` bytes; recv holds world * bytes, rank-major
 *   all_reduce_max_i64  element-wise maximum over the ranks of n int64 values, in place
 *   all_to_all_v        send_bytes[p] bytes at send + send_off[p] go to rank p; recv_bytes[p] bytes from rank p land at
 *                       recv + recv_off[p] (the counts were agreed by an all_gather before) */
typedef struct pandrs_hip_transport {
    void *user;
    int32_t (*all_gather)(void *user, const void *send, void *recv, int64_t bytes);
    int32_t (*all_reduce_max_i64)(void *user, int64_t *vals, int32_t n);
    int32_t (*all_to_all_v)(void *user, const void *send, const int64_t *send_bytes, const int64_t *send_off,
                            void *recv, const int64_t *recv_bytes, const int64_t *recv_off);
} pandrs_hip_transport;
int32_t pandrs_hip_comm_adopt_transport(const pandrs_hip_transport *transport, int32_t rank, int32_t world, pandrs_hip_comm **out_comm);
int32_t pandrs_hip_comm_destroy(pandrs_hip_comm *comm);

/* Row-range-sharded group_by(..).aggregate(..) (aggregation.rs:763) over all ranks' rows: local partial states ->
 * owner split (one block of records per owner, a small column store; no host round trip) -> count exchange straight from the
 * device counts -> ONE grouped ncclSend / ncclRecv all-to-all, a block per peer, on the context's stream -> merge.  The result (fetch with groupby_fetch) holds the groups this rank owns; the ranks' key sets are
 * disjoint.  That is the path for Sum / Mean / Min / Max / Count over one key column.  Anything else except First / Last
 * (Std / Var / Median / Nunique, composite keys of up to 8 columns) takes the row shuffle inside the same call: every row
 * goes to the owner of its key (the radix partitioner with P = world; a composite key on a hash cell of the tuple), one count
 * exchange, one grouped all-to-all of all columns, and the owner runs the ordinary groupby on what it received.
 * Null-mask presence may differ between ranks: the layout (which value columns carry a non-null count) is agreed ON the
 * count exchange — every rank plans with the layout of the previous call of this shape plus its own masks, and the ranks
 * repeat their local phase once when they find they disagreed — so a steady-state call makes no collective of its own
 * for it (at most 62 value columns on this path).  A rank whose local phase fails still joins the count exchange with its
 * status: EVERY rank then returns an error (nobody is left blocked in a collective).  A failure that is rank-local AFTER
 * the count exchange (the receive buffer cannot be allocated) aborts the communicator (ncclCommAbort) so that the peers
 * return instead of blocking; the communicator then refuses further calls (PANDRS_HIP_ERR_NOT_INITIALIZED).  The exchange
 * buffers live in the communicator and are only ever grown. */
int32_t pandrs_hip_dist_groupby_agg(pandrs_hip_ctx *ctx, pandrs_hip_comm *comm, int32_t mem_space,
                                    const pandrs_hip_column *keys, int32_t n_keys, int64_t n_rows,
                                    const pandrs_hip_column *vals, int32_t n_vals,
                                    const pandrs_hip_agg_spec *aggs, int32_t n_aggs, int64_t *out_n_groups);

/* BASELINE config 5 across ranks: inner_join (join.rs:32) of row-range-sharded sides + group_by(g).sum(v).  The
 * build (right) side is all-gathered, the probe side stays on its GPU, the local fused result goes through the
 * groupby exchange.  Device-resident shards, 8-byte build-side columns. */
int32_t pandrs_hip_dist_join_groupby_sum(pandrs_hip_ctx *ctx, pandrs_hip_comm *comm, int32_t mem_space,
                                         const pandrs_hip_column *left_key, const pandrs_hip_column *left_val, int64_t n_left,
                                         const pandrs_hip_column *right_key, const pandrs_hip_column *right_group, int64_t n_right,
                                         int64_t *out_n_groups);

/* Everything K1's three families of reference functions need, from ONE pass over the column:
 *  (A) OptimizedDataFrame::{sum,mean,min,max}  (src/optimized/split_dataframe/aggregate.rs:21-215): values as f64
 *      ((v as f64) for Int64), sum = sum_f64 (0.0 when count == 0), mean = sum_f64 / count and min / max = `min` /
 *      `max` (fold with f64::min / f64::max from +-inf: NaN operands are ignored, infinities are not), each
 *      Err(Error::Empty) when count == 0;
 *  (B) Float64Column::{sum,mean,min,max} (src/column/float64_column.rs:100-199) and Int64Column's
 *      (src/column/int64_column.rs:100-199): min / max skip NON-FINITE values -> `min_finite` / `max_finite`, None when
 *      count_finite == 0; Int64Column::sum is the wrapping i64 sum `sum_i64`, its mean sum_i64 as f64 / count;
 *  (C) simd_{sum,mean,min,max}_{f64,i64} (src/optimized/jit/simd.rs:9-112): simd_mean_i64 is the INTEGER division
 *      sum_i64 / count (:77-82), empties give 0 / 0.0 and the fold identities (+-inf, i64::MAX / MIN).
 * f64 sums are accumulated pairwise on the device (the reference: Kahan per chunk + Kahan combine,
 * src/optimized/jit/parallel.rs:71-102); they agree to 1e-9 relative, not bit for bit.
 * +0.0 / -0.0 ties: -0.0 < +0.0 here; f64::min leaves the tie unspecified. */
typedef struct pandrs_hip_column_stats {
    int64_t count;          /* non-null values */
    int64_t count_finite;   /* f64: finite ones among them; i64: = count */
    double sum_f64;         /* sum of the values as f64 */
    double sum_sq;          /* sum of their squares as f64 */
    int64_t sum_i64;        /* i64 columns: wrapping integer sum; 0 for f64 columns */
    int64_t min_i64, max_i64; /* i64 columns: exact extremes (i64::MAX / MIN when count == 0); 0 for f64 columns */
    double min, max;        /* NaN-ignoring extremes over the non-null values; +inf / -inf when there is none; i64: as f64 */
    double min_finite, max_finite; /* the same over finite values only */
} pandrs_hip_column_stats;

int32_t pandrs_hip_reduce_stats(pandrs_hip_ctx *ctx, int32_t mem_space,
                                const pandrs_hip_column *col, int64_t n, pandrs_hip_column_stats *out);

#ifdef __cplusplus
}
#endif
#endif /* PANDRS_HIP_H */
