// predicate.hip — row masks of one column built on the device, behind PandasCompatExt::gt / ge / lt / le / eq_value / ne_value
// (reference src/dataframe/pandas_compat/helpers/comparison_ops.rs:7-46), between (functions.rs:253-257), is_between (:4141-4161),
// isna / notna (:930-933, :1312-1315), is_finite / is_infinite (:4016-4024) and isin / isin_numeric (:141-158), gfx950, wave64.
//
// The output is the data of a BOOLBITS column without a null mask: bit = 1, the row is selected; pandrs_hip_filter_indices takes it
// in place.  Rows in tiles of PRED_TILE; row p0 + r * 256 + tid, so every load is coalesced and one wave ballot IS the 64-row word,
// stored bytewise by lanes 0 .. 7 (no byte at or past ceil(n / 8) is touched, the output may sit at any byte offset).
// 1. Compare: one stream over the column and its mask; every compare happens in f64, as the reference's
//    get_column_numeric_values has it; a null cell is NaN.  F64: the kernel is instantiated per op.  I64: (double)v is monotone
//    in v, so what an op selects is an interval of integers (NE: the complement of one); the host finds its ends by bisection
//    with the very expression the F64 kernel evaluates, and the stream compares integers: the same bits as converting every
//    cell, without the conversion's instructions in the loop ("predicate_path" 1 converts per row instead: the A/B of
//    experiments/predicate_bench.py, and the tests hold the two equal).
// 2. isin, LDS set: every workgroup builds an open-addressing table of the value list's 64-bit keys in LDS (64-bit compare-and-swap)
//    and probes it linearly per row.  Any 64-bit pattern can be a key, so the empty marker (all ones) is never stored: "the marker
//    is in the set" is one flag.
// 3. isin, global set (lists beyond PRED_LDS_VALUES): one kernel builds the same table in the workspace, a second one probes it.
//    The kernel boundary is the only hand-off: no workgroup waits for another.  Every probe and insert loop is bounded by the slot
//    count.
#include "engine.hpp"

#include <algorithm>
#include <cfloat>

namespace pandrs {

#pragma clang fp contract(off)      // EQ / NE are the reference's |v - a| against EPSILON, the subtraction rounded on its own

constexpr int PRED_THREADS = 256;                       // 4 waves
constexpr int PRED_RPT = 8;                             // rows per thread in a tile
constexpr int PRED_TILE = PRED_THREADS * PRED_RPT;      // 2048 rows: predicate_tile_rows of pandrs_hip.h
constexpr int PRED_BLOCKS_PER_CU = 4;                   // predicate_blocks_per_cu of pandrs_hip.h
constexpr int64_t PRED_LDS_VALUES = 4096;               // isin_lds_max_values of pandrs_hip.h: 8192 slots x 8 bytes = 64 KiB of table (+ PRED_LDS_EXTRA)
constexpr int PRED_LDS_EXTRA = 64;                      // behind the LDS table: the marker flag and the waves' counts
constexpr uint32_t PRED_SEED = 0x1B873593u;
constexpr int64_t PRED_MAX_VALUES = int64_t(1) << 30;   // the slot count stays a uint32

struct PredCol {
    const void *data;
    const uint8_t *mask;    // null bits or nullptr
    int64_t n;
};

struct PredOut {
    uint8_t *bits;                  // ceil(n / 8) bytes or nullptr (count only)
    unsigned long long *count;      // += the selected rows
};

// the 64-row word `b` that starts at row `row0`, written bytewise: lanes 0 .. 7 hold one byte each, and no byte at or past
// ceil(n / 8) is touched (rows past n are never selected, so the last byte's high bits are 0)
__device__ __forceinline__ void pred_store_word(uint8_t *bits, int64_t row0, int64_t n, uint64_t b, uint32_t lane) {
    const int64_t byte = (row0 >> 3) + lane;
    if (lane < 8 && byte < ((n + 7) >> 3)) bits[byte] = (uint8_t)(b >> (lane * 8));
}

// the waves' popcounts -> one atomic add per workgroup; `s_cnt` holds one slot per wave
__device__ __forceinline__ void pred_add_count(unsigned long long *count, uint32_t mine, uint32_t *s_cnt) {
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (lane == 0) s_cnt[wave] = mine;
    __syncthreads();
    if (tid == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < PRED_THREADS / 64; w++) s += s_cnt[w];
        if (s) atomicAdd(count, s);
    }
}

__host__ __device__ __forceinline__ uint64_t pred_bits(double v) {
    uint64_t b;
    __builtin_memcpy(&b, &v, 8);
    return b;
}
__host__ __device__ __forceinline__ bool pred_is_nan(double v) {
    return (pred_bits(v) & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull;
}

template <int OP>
__host__ __device__ __forceinline__ bool pred_eval(double v, double a, double b) {
    const uint64_t mag = pred_bits(v) & 0x7FFFFFFFFFFFFFFFull;
    switch (OP) {
    case PANDRS_HIP_PRED_GT: return !pred_is_nan(v) && v > a;                                   // comparison_ops.rs:9
    case PANDRS_HIP_PRED_GE: return !pred_is_nan(v) && v >= a;                                  // :15
    case PANDRS_HIP_PRED_LT: return !pred_is_nan(v) && v < a;                                   // :21
    case PANDRS_HIP_PRED_LE: return !pred_is_nan(v) && v <= a;                                  // :27
    case PANDRS_HIP_PRED_EQ: return !pred_is_nan(v) && fabs(v - a) < DBL_EPSILON;               // :35
    case PANDRS_HIP_PRED_NE: return pred_is_nan(v) || fabs(v - a) >= DBL_EPSILON;               // :44
    case PANDRS_HIP_PRED_BETWEEN: return v >= a && v <= b;                                      // functions.rs:255
    case PANDRS_HIP_PRED_BETWEEN_EXCLUSIVE: return !pred_is_nan(v) && v > a && v < b;           // functions.rs:4157
    case PANDRS_HIP_PRED_ISNA: return mag > 0x7FF0000000000000ull;
    case PANDRS_HIP_PRED_NOTNA: return mag <= 0x7FF0000000000000ull;
    case PANDRS_HIP_PRED_IS_FINITE: return mag < 0x7FF0000000000000ull;
    default: return mag == 0x7FF0000000000000ull;                                               // IS_INFINITE
    }
}

// what pred_eval does on the host: the bisection of the I64 path asks it about single cells
static bool pred_eval_host(int op, double v, double a, double b) {
    switch (op) {
    case PANDRS_HIP_PRED_GT: return pred_eval<PANDRS_HIP_PRED_GT>(v, a, b);
    case PANDRS_HIP_PRED_GE: return pred_eval<PANDRS_HIP_PRED_GE>(v, a, b);
    case PANDRS_HIP_PRED_LT: return pred_eval<PANDRS_HIP_PRED_LT>(v, a, b);
    case PANDRS_HIP_PRED_LE: return pred_eval<PANDRS_HIP_PRED_LE>(v, a, b);
    case PANDRS_HIP_PRED_EQ: return pred_eval<PANDRS_HIP_PRED_EQ>(v, a, b);
    case PANDRS_HIP_PRED_NE: return pred_eval<PANDRS_HIP_PRED_NE>(v, a, b);
    case PANDRS_HIP_PRED_BETWEEN: return pred_eval<PANDRS_HIP_PRED_BETWEEN>(v, a, b);
    case PANDRS_HIP_PRED_BETWEEN_EXCLUSIVE: return pred_eval<PANDRS_HIP_PRED_BETWEEN_EXCLUSIVE>(v, a, b);
    case PANDRS_HIP_PRED_ISNA: return pred_eval<PANDRS_HIP_PRED_ISNA>(v, a, b);
    case PANDRS_HIP_PRED_NOTNA: return pred_eval<PANDRS_HIP_PRED_NOTNA>(v, a, b);
    case PANDRS_HIP_PRED_IS_FINITE: return pred_eval<PANDRS_HIP_PRED_IS_FINITE>(v, a, b);
    default: return pred_eval<PANDRS_HIP_PRED_IS_INFINITE>(v, a, b);
    }
}

// the tile's null-mask bytes, one per row of this thread (0 without a mask): in flight together with the cells
__device__ __forceinline__ void pred_load_nulls(const PredCol &c, int64_t p0, uint32_t tid, uint8_t (&nb)[PRED_RPT]) {
#pragma unroll
    for (int r = 0; r < PRED_RPT; r++) {
        const int64_t p = p0 + r * PRED_THREADS + tid;
        nb[r] = c.mask && p < c.n ? c.mask[p >> 3] : 0;
    }
}

template <bool IS_I64, int OP>
__global__ __launch_bounds__(PRED_THREADS) void pred_compare_kernel(PredCol c, int64_t tiles, double a, double b, PredOut o) {
    __shared__ uint32_t s_cnt[PRED_THREADS / 64];
    const uint64_t *__restrict__ data = static_cast<const uint64_t *>(c.data);
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    uint32_t selected = 0;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t p0 = t * PRED_TILE;
        uint64_t cell[PRED_RPT];
        uint8_t nb[PRED_RPT];
#pragma unroll
        for (int r = 0; r < PRED_RPT; r++) {            // every load of the tile in flight before the first ballot
            const int64_t p = p0 + r * PRED_THREADS + tid;
            cell[r] = p < c.n ? data[p] : 0;
        }
        pred_load_nulls(c, p0, tid, nb);
#pragma unroll
        for (int r = 0; r < PRED_RPT; r++) {            // (a uniform loop: the ballots see every lane)
            const int64_t p = p0 + r * PRED_THREADS + tid;
            const bool in = p < c.n;
            double v = IS_I64 ? (double)(int64_t)cell[r] : __longlong_as_double((long long)cell[r]);
            if ((nb[r] >> (p & 7)) & 1) v = __longlong_as_double((long long)CANON_NAN);         // a null cell behaves as NaN
            const uint64_t w = __ballot(in && pred_eval<OP>(v, a, b));
            if (o.bits) pred_store_word(o.bits, p - lane, c.n, w, lane);
            if (lane == 0) selected += (uint32_t)__popcll(w);
        }
    }
    pred_add_count(o.count, selected, s_cnt);
}

// I64: a cell is selected when (lo <= v && v <= hi) != invert; a null cell when null_sel.  lo > hi is the empty interval.
struct PredRange {
    int64_t lo, hi;
    int invert, null_sel;
};

__global__ __launch_bounds__(PRED_THREADS) void pred_range_kernel(PredCol c, int64_t tiles, PredRange g, PredOut o) {
    __shared__ uint32_t s_cnt[PRED_THREADS / 64];
    const int64_t *__restrict__ data = static_cast<const int64_t *>(c.data);
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    uint32_t selected = 0;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t p0 = t * PRED_TILE;
        int64_t cell[PRED_RPT];
        uint8_t nb[PRED_RPT];
#pragma unroll
        for (int r = 0; r < PRED_RPT; r++) {
            const int64_t p = p0 + r * PRED_THREADS + tid;
            cell[r] = p < c.n ? data[p] : 0;
        }
        pred_load_nulls(c, p0, tid, nb);
#pragma unroll
        for (int r = 0; r < PRED_RPT; r++) {            // (a uniform loop: the ballots see every lane)
            const int64_t p = p0 + r * PRED_THREADS + tid;
            const bool inside = cell[r] >= g.lo && cell[r] <= g.hi;
            const bool sel = (nb[r] >> (p & 7)) & 1 ? g.null_sel != 0 : inside != (g.invert != 0);
            const uint64_t w = __ballot(p < c.n && sel);
            if (o.bits) pred_store_word(o.bits, p - lane, c.n, w, lane);
            if (lane == 0) selected += (uint32_t)__popcll(w);
        }
    }
    pred_add_count(o.count, selected, s_cnt);
}

// The first int64 for which the monotone `upper` holds (false ... false true ... true over ascending v), or false when it never does.
template <typename F>
static bool pred_first(F upper, int64_t *out) {
    int64_t lo = INT64_MIN, hi = INT64_MAX;
    if (!upper(hi)) return false;
    while (lo < hi) {
        const int64_t mid = lo + (int64_t)(((uint64_t)hi - (uint64_t)lo) >> 1);
        if (upper(mid)) hi = mid; else lo = mid + 1;
    }
    *out = lo;
    return true;
}
// The last int64 for which the monotone `lower` holds (true ... true false ... false), or false when it never does.
template <typename F>
static bool pred_last(F lower, int64_t *out) {
    int64_t lo = INT64_MIN, hi = INT64_MAX;
    if (!lower(lo)) return false;
    while (lo < hi) {
        const int64_t mid = hi - (int64_t)(((uint64_t)hi - (uint64_t)lo) >> 1);
        if (lower(mid)) lo = mid; else hi = mid - 1;
    }
    *out = lo;
    return true;
}

// What `op` selects among the int64 cells, as an interval.  (double)v never decreases as v grows, and neither does (double)v - a, so
// every op is the meet of an upper set and a lower set of v, each bounded by bisection over pred_eval itself; NE is the complement
// of EQ's interval unless a is NaN (then v - a is NaN and NE, like EQ, is false).  A null cell is NaN: pred_eval answers it too.
static PredRange pred_range(int op, double a, double b) {
    const double nan = __builtin_nan("");
    PredRange g{1, 0, 0, pred_eval_host(op, nan, a, b) ? 1 : 0};
    auto as = [](int64_t v) { return (double)v; };
    int64_t lo = INT64_MIN, hi = INT64_MAX;
    bool some = true;
    switch (op) {
    case PANDRS_HIP_PRED_GT: case PANDRS_HIP_PRED_GE:
        some = pred_first([&](int64_t v) { return pred_eval_host(op, as(v), a, b); }, &lo);
        break;
    case PANDRS_HIP_PRED_LT: case PANDRS_HIP_PRED_LE:
        some = pred_last([&](int64_t v) { return pred_eval_host(op, as(v), a, b); }, &hi);
        break;
    case PANDRS_HIP_PRED_BETWEEN:
        some = pred_first([&](int64_t v) { return as(v) >= a; }, &lo) && pred_last([&](int64_t v) { return as(v) <= b; }, &hi);
        break;
    case PANDRS_HIP_PRED_BETWEEN_EXCLUSIVE:
        some = pred_first([&](int64_t v) { return as(v) > a; }, &lo) && pred_last([&](int64_t v) { return as(v) < b; }, &hi);
        break;
    case PANDRS_HIP_PRED_EQ: case PANDRS_HIP_PRED_NE:
        // fabs(x) < EPSILON is -EPSILON < x && x < EPSILON, x = (double)v - a
        some = pred_first([&](int64_t v) { return as(v) - a > -DBL_EPSILON; }, &lo) && pred_last([&](int64_t v) { return as(v) - a < DBL_EPSILON; }, &hi);
        if (op == PANDRS_HIP_PRED_NE) {
            if (a != a) return g;                       // nothing but the null cells
            g.invert = 1;
        }
        break;
    default:                                            // ISNA .. IS_INFINITE: a converted int64 is a finite number
        some = pred_eval_host(op, 0.0, a, b);
        break;
    }
    if (some && lo <= hi) { g.lo = lo; g.hi = hi; }
    return g;
}

// ---- isin ----------------------------------------------------------------------------------------------------------------
// KEY: how a cell becomes its 64-bit key.  0 = the 8 bytes as they are (F64 bits, or I64 against an I64 list), 1 = the bits of
// (double)v for an I64 cell against an F64 list (functions.rs:151-155 through get_column_numeric_values), 2 = a u32 pool code.
template <int KEY>
__device__ __forceinline__ uint64_t pred_key(const void *data, int64_t p) {
    if (KEY == 2) return static_cast<const uint32_t *>(data)[p];
    const uint64_t x = static_cast<const uint64_t *>(data)[p];
    return KEY == 1 ? (uint64_t)__double_as_longlong((double)(int64_t)x) : x;
}

struct PredSet {
    const void *values;             // the list: 8-byte cells, or u32 codes (values32)
    int64_t n_values;
    int values32;
    uint32_t slots;                 // a power of two >= 2 x n_values (and >= 2)
    unsigned long long *table;      // global set: slots cells, EMPTY_KEY where free (LDS set: unused)
    uint32_t *has_marker;           // global set: != 0 when EMPTY_KEY itself is listed
};

__device__ __forceinline__ uint64_t pred_value(const PredSet &s, int64_t i) {
    return s.values32 ? (uint64_t)static_cast<const uint32_t *>(s.values)[i] : static_cast<const uint64_t *>(s.values)[i];
}
// (the project's key mixer: integral f64 values differ in their high bits only, a low-bits hash would chain them)
__device__ __forceinline__ uint32_t pred_slot(uint64_t k, uint32_t slots) { return slot_of(hash32(k, PRED_SEED), slots); }

// inserts k (never EMPTY_KEY) into an open-addressing table; at most `slots` steps
__device__ __forceinline__ void pred_insert(unsigned long long *table, uint32_t slots, uint64_t k) {
    uint32_t s = pred_slot(k, slots);
    for (uint32_t j = 0; j < slots; j++) {
        const unsigned long long old = atomicCAS(&table[s], (unsigned long long)EMPTY_KEY, (unsigned long long)k);
        if (old == EMPTY_KEY || old == k) return;
        s = (s + 1) & (slots - 1);
    }
}
// whether k (never EMPTY_KEY) is in the table; at most `slots` steps
__device__ __forceinline__ bool pred_lookup(const unsigned long long *table, uint32_t slots, uint64_t k) {
    uint32_t s = pred_slot(k, slots);
    for (uint32_t j = 0; j < slots; j++) {
        const unsigned long long t = table[s];
        if (t == k) return true;
        if (t == EMPTY_KEY) return false;
        s = (s + 1) & (slots - 1);
    }
    return false;
}

// the probe stream both sets share
template <int KEY>
__device__ __forceinline__ uint32_t pred_probe_tiles(const PredCol &c, int64_t tiles, const unsigned long long *table, uint32_t slots,
                                                     bool has_marker, int negate, const PredOut &o) {
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    uint32_t selected = 0;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t p0 = t * PRED_TILE;
        uint64_t key[PRED_RPT];
        uint8_t nb[PRED_RPT];
#pragma unroll
        for (int r = 0; r < PRED_RPT; r++) {
            const int64_t p = p0 + r * PRED_THREADS + tid;
            key[r] = p < c.n ? pred_key<KEY>(c.data, p) : 0;
        }
        pred_load_nulls(c, p0, tid, nb);
#pragma unroll
        for (int r = 0; r < PRED_RPT; r++) {            // (a uniform loop: the ballots see every lane)
            const int64_t p = p0 + r * PRED_THREADS + tid;
            const bool in = p < c.n;
            bool hit = false;
            if (in && !((nb[r] >> (p & 7)) & 1))        // a null cell never matches
                hit = key[r] == EMPTY_KEY ? has_marker : pred_lookup(table, slots, key[r]);
            const uint64_t w = __ballot(in && (hit != (negate != 0)));
            if (o.bits) pred_store_word(o.bits, p - lane, c.n, w, lane);
            if (lane == 0) selected += (uint32_t)__popcll(w);
        }
    }
    return selected;
}

// dynamic LDS: slots x 8 bytes of table, then PRED_LDS_EXTRA bytes (the marker flag, the waves' counts)
template <int KEY>
__global__ __launch_bounds__(PRED_THREADS) void pred_isin_lds_kernel(PredCol c, int64_t tiles, PredSet s, int negate, PredOut o) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pred_smem[];
    unsigned long long *table = reinterpret_cast<unsigned long long *>(pred_smem);
    uint32_t *extra = reinterpret_cast<uint32_t *>(pred_smem + (size_t)s.slots * 8);     // [0] marker flag, [1 .. 4] counts
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < s.slots; i += PRED_THREADS) table[i] = EMPTY_KEY;
    if (tid == 0) extra[0] = 0;
    __syncthreads();
    for (int64_t i = tid; i < s.n_values; i += PRED_THREADS) {
        const uint64_t k = pred_value(s, i);
        if (k == EMPTY_KEY) extra[0] = 1;               // (every writer writes 1)
        else pred_insert(table, s.slots, k);
    }
    __syncthreads();
    const uint32_t selected = pred_probe_tiles<KEY>(c, tiles, table, s.slots, extra[0] != 0, negate, o);
    pred_add_count(o.count, selected, extra + 1);
}

__global__ __launch_bounds__(PRED_THREADS) void pred_isin_build_kernel(PredSet s) {
    for (int64_t i = (int64_t)blockIdx.x * PRED_THREADS + threadIdx.x; i < s.n_values; i += (int64_t)gridDim.x * PRED_THREADS) {
        const uint64_t k = pred_value(s, i);
        if (k == EMPTY_KEY) atomicOr(s.has_marker, 1u);
        else pred_insert(s.table, s.slots, k);
    }
}

template <int KEY>
__global__ __launch_bounds__(PRED_THREADS) void pred_isin_probe_kernel(PredCol c, int64_t tiles, PredSet s, int negate, PredOut o) {
    __shared__ uint32_t s_cnt[PRED_THREADS / 64];
    const uint32_t selected = pred_probe_tiles<KEY>(c, tiles, s.table, s.slots, *s.has_marker != 0, negate, o);
    pred_add_count(o.count, selected, s_cnt);
}

template <bool IS_I64, int OP>
static void pred_launch(pandrs_hip_ctx *c, int grid, const PredCol &pc, int64_t tiles, double a, double b, const PredOut &po) {
    hipLaunchKernelGGL((pred_compare_kernel<IS_I64, OP>), dim3(grid), dim3(PRED_THREADS), 0, c->stream, pc, tiles, a, b, po);
}
template <bool IS_I64>
static void pred_launch_op(pandrs_hip_ctx *c, int op, int grid, const PredCol &pc, int64_t tiles, double a, double b, const PredOut &po) {
    switch (op) {
    case PANDRS_HIP_PRED_GT: pred_launch<IS_I64, PANDRS_HIP_PRED_GT>(c, grid, pc, tiles, a, b, po); break;
    case PANDRS_HIP_PRED_GE: pred_launch<IS_I64, PANDRS_HIP_PRED_GE>(c, grid, pc, tiles, a, b, po); break;
    case PANDRS_HIP_PRED_LT: pred_launch<IS_I64, PANDRS_HIP_PRED_LT>(c, grid, pc, tiles, a, b, po); break;
    case PANDRS_HIP_PRED_LE: pred_launch<IS_I64, PANDRS_HIP_PRED_LE>(c, grid, pc, tiles, a, b, po); break;
    case PANDRS_HIP_PRED_EQ: pred_launch<IS_I64, PANDRS_HIP_PRED_EQ>(c, grid, pc, tiles, a, b, po); break;
    case PANDRS_HIP_PRED_NE: pred_launch<IS_I64, PANDRS_HIP_PRED_NE>(c, grid, pc, tiles, a, b, po); break;
    case PANDRS_HIP_PRED_BETWEEN: pred_launch<IS_I64, PANDRS_HIP_PRED_BETWEEN>(c, grid, pc, tiles, a, b, po); break;
    case PANDRS_HIP_PRED_BETWEEN_EXCLUSIVE: pred_launch<IS_I64, PANDRS_HIP_PRED_BETWEEN_EXCLUSIVE>(c, grid, pc, tiles, a, b, po); break;
    case PANDRS_HIP_PRED_ISNA: pred_launch<IS_I64, PANDRS_HIP_PRED_ISNA>(c, grid, pc, tiles, a, b, po); break;
    case PANDRS_HIP_PRED_NOTNA: pred_launch<IS_I64, PANDRS_HIP_PRED_NOTNA>(c, grid, pc, tiles, a, b, po); break;
    case PANDRS_HIP_PRED_IS_FINITE: pred_launch<IS_I64, PANDRS_HIP_PRED_IS_FINITE>(c, grid, pc, tiles, a, b, po); break;
    default: pred_launch<IS_I64, PANDRS_HIP_PRED_IS_INFINITE>(c, grid, pc, tiles, a, b, po); break;
    }
}

// what both entry points share once their arguments are checked: the output slot and the counter read-back
struct PredCall {
    pandrs_hip_ctx *c;
    size_t nbytes;
    uint8_t *out_bits;
    int64_t *out_count;
    int32_t finish(Stager &stg, unsigned long long *d_count) {
        ST_TRY(stg.copy_back(nbytes));
        unsigned long long count = 0;
        HIP_TRY(hipMemcpyAsync(&count, d_count, 8, hipMemcpyDeviceToHost, c->stream));
        ST_TRY(timings_end(c));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (out_count) *out_count = (int64_t)count;
        return 0;
    }
};

static int32_t pred_check_common(const char *entry, pandrs_hip_ctx *c, const pandrs_hip_column *col, int64_t n_rows, uint8_t *out_bits,
                                 int64_t *out_count) {
    if (!c || !col || n_rows < 0 || (n_rows > 0 && !col->data) || (!out_bits && !out_count))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "%s: bad arguments", entry);
    return 0;
}

int32_t predicate_entry(pandrs_hip_ctx *c, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows, int32_t op, double a, double b,
                        int32_t out_mem_space, uint8_t *out_bits, int64_t *out_count) {
    ST_TRY(pred_check_common("predicate", c, col, n_rows, out_bits, out_count));
    ST_TRY(check_mem_space("predicate", mem_space, out_bits ? out_mem_space : PANDRS_HIP_MEM_DEVICE));   // (no output, no output space)
    if (op < PANDRS_HIP_PRED_GT || op > PANDRS_HIP_PRED_IS_INFINITE)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "predicate: op %d is not a pandrs_hip_pred_op", op);
    if (col->dtype != PANDRS_HIP_I64 && col->dtype != PANDRS_HIP_F64)
        return fail(PANDRS_HIP_ERR_TYPE_MISMATCH, "predicate: the column has dtype %d, expected I64 or F64", col->dtype);
    if (n_rows >= (int64_t(1) << 32))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "predicate: %lld rows; one call takes fewer than 2^32", (long long)n_rows);
    if (out_count) *out_count = 0;
    if (n_rows == 0) return 0;
    const size_t nbytes = ((size_t)n_rows + 7) / 8;
    std::lock_guard<std::mutex> lock(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    timings_begin(c);

    ColView cv{col->data, col->null_mask};
    uint8_t *d_bits = out_bits;
    Stager stg{c, mem_space, out_mem_space};
    if (const size_t need = stg.col_size(*col, n_rows) + stg.out_size(out_bits, nbytes)) {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_STAGE_IN);
        ST_TRY(stg.reserve(need));
        cv = stg.col(*col, n_rows);
        d_bits = stg.out(out_bits, nbytes);
        if (stg.status) return stg.status;
    }
    if (reinterpret_cast<uintptr_t>(cv.data) & 7)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "predicate: the column must be 8-byte aligned");
    ST_TRY(c->work.ensure(Arena::padded(8), c->stream));
    unsigned long long *d_count = c->work.take<unsigned long long>(1);
    if (!d_count) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (predicate)");

    const int64_t tiles = (n_rows + PRED_TILE - 1) / PRED_TILE;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)c->n_cu * PRED_BLOCKS_PER_CU, tiles));
    const PredCol pc{cv.data, cv.mask, n_rows};
    const PredOut po{d_bits, d_count};
    {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_AGGREGATE);
        HIP_TRY(hipMemsetAsync(d_count, 0, 8, c->stream));
        if (col->dtype == PANDRS_HIP_I64 && c->opt.predicate_path == 1) pred_launch_op<true>(c, op, grid, pc, tiles, a, b, po);   // A/B: convert per row
        else if (col->dtype == PANDRS_HIP_I64)
            hipLaunchKernelGGL(pred_range_kernel, dim3(grid), dim3(PRED_THREADS), 0, c->stream, pc, tiles, pred_range(op, a, b), po);
        else pred_launch_op<false>(c, op, grid, pc, tiles, a, b, po);
        HIP_TRY(hipGetLastError());
    }
    c->timings.algorithmic_bytes = (int64_t)n_rows * 8 + (cv.mask ? (int64_t)nbytes : 0) + (d_bits ? (int64_t)nbytes : 0);
    PredCall call{c, nbytes, out_bits, out_count};
    return call.finish(stg, d_count);
}

template <int KEY>
static int32_t pred_launch_isin(pandrs_hip_ctx *c, bool lds, int grid, const PredCol &pc, int64_t tiles, const PredSet &ps, int negate,
                                const PredOut &po) {
    if (lds) {
        const size_t bytes = (size_t)ps.slots * 8 + PRED_LDS_EXTRA;
        static std::atomic<bool> raised{false};         // once per instantiation: the largest set this kernel is ever launched with
        if (!raised.load()) {
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(pred_isin_lds_kernel<KEY>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)(PRED_LDS_VALUES * 16 + PRED_LDS_EXTRA)));
            raised.store(true);
        }
        hipLaunchKernelGGL((pred_isin_lds_kernel<KEY>), dim3(grid), dim3(PRED_THREADS), bytes, c->stream, pc, tiles, ps, negate, po);
    } else {
        hipLaunchKernelGGL((pred_isin_probe_kernel<KEY>), dim3(grid), dim3(PRED_THREADS), 0, c->stream, pc, tiles, ps, negate, po);
    }
    return 0;
}

int32_t isin_entry(pandrs_hip_ctx *c, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows, int32_t values_mem_space,
                   const pandrs_hip_column *values, int64_t n_values, int32_t negate, int32_t out_mem_space, uint8_t *out_bits,
                   int64_t *out_count) {
    ST_TRY(pred_check_common("isin", c, col, n_rows, out_bits, out_count));
    if (!values || n_values < 0 || (n_values > 0 && !values->data)) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "isin: bad value list");
    ST_TRY(check_mem_space("isin", mem_space, out_bits ? out_mem_space : PANDRS_HIP_MEM_DEVICE));
    ST_TRY(check_mem_space("isin", values_mem_space));
    int key = -1;
    if (col->dtype == PANDRS_HIP_F64 && values->dtype == PANDRS_HIP_F64) key = 0;
    else if (col->dtype == PANDRS_HIP_I64 && values->dtype == PANDRS_HIP_I64) key = 0;
    else if (col->dtype == PANDRS_HIP_I64 && values->dtype == PANDRS_HIP_F64) key = 1;
    else if (col->dtype == PANDRS_HIP_U32CODE && values->dtype == PANDRS_HIP_U32CODE) key = 2;
    if (key < 0)
        return fail(PANDRS_HIP_ERR_TYPE_MISMATCH, "isin: a column of dtype %d against values of dtype %d (F64 / F64, I64 / F64, I64 / I64 or U32CODE / U32CODE)",
                    col->dtype, values->dtype);
    if (values->null_mask) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "isin: the value list takes no null mask");
    if (n_rows >= (int64_t(1) << 32))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "isin: %lld rows; one call takes fewer than 2^32", (long long)n_rows);
    if (n_values > PRED_MAX_VALUES)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "isin: %lld values; one call takes at most 2^30", (long long)n_values);
    if (out_count) *out_count = 0;
    if (n_rows == 0) return 0;
    const size_t nbytes = ((size_t)n_rows + 7) / 8;
    std::lock_guard<std::mutex> lock(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    timings_begin(c);

    const bool lds = c->opt.isin_path == 2 ? false : n_values <= PRED_LDS_VALUES;      // 0 and 1: the LDS set wherever it fits
    uint32_t slots = 2;
    while ((int64_t)slots < 2 * n_values) slots <<= 1;

    // ---- staging (both inputs and a host output) and the workspace (the counter, the flag, the global table), sized up front ----
    ColView cv{col->data, col->null_mask};
    const void *d_values = values->data;
    uint8_t *d_bits = out_bits;
    Stager stg{c, mem_space, out_mem_space}, vstg{c, values_mem_space};
    const size_t vbytes = dtype_bytes(values->dtype, n_values);
    if (const size_t need = stg.col_size(*col, n_rows) + stg.out_size(out_bits, nbytes) + vstg.in_size(values->data, vbytes)) {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_STAGE_IN);
        ST_TRY(stg.reserve(need));                      // (one arena: vstg takes its slot from the same reservation)
        cv = stg.col(*col, n_rows);
        d_bits = stg.out(out_bits, nbytes);
        d_values = vstg.in(values->data, vbytes);
        if (stg.status) return stg.status;
        if (vstg.status) return vstg.status;
    }
    const uintptr_t align = key == 2 ? 3 : 7;
    if ((reinterpret_cast<uintptr_t>(cv.data) | (n_values ? reinterpret_cast<uintptr_t>(d_values) : 0)) & align)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "isin: the column and the values must be %d-byte aligned", (int)align + 1);
    ST_TRY(c->work.ensure(Arena::padded(8) + Arena::padded(4) + (lds ? 0 : Arena::padded((size_t)slots * 8)), c->stream));
    unsigned long long *d_count = c->work.take<unsigned long long>(1);
    uint32_t *d_flag = c->work.take<uint32_t>(1);
    unsigned long long *d_table = lds ? nullptr : c->work.take<unsigned long long>(slots);
    if (!d_count || !d_flag || (!lds && !d_table)) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (isin)");

    const int64_t tiles = (n_rows + PRED_TILE - 1) / PRED_TILE;
    // an LDS table beyond 32 KiB leaves room for two workgroups per CU, a smaller one for four
    const int per_cu = lds && (size_t)slots * 8 > 32 * 1024 ? 2 : PRED_BLOCKS_PER_CU;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)c->n_cu * per_cu, tiles));
    const PredCol pc{cv.data, cv.mask, n_rows};
    const PredOut po{d_bits, d_count};
    const PredSet ps{d_values, n_values, key == 2 ? 1 : 0, slots, d_table, d_flag};
    HIP_TRY(hipMemsetAsync(d_count, 0, 8, c->stream));
    if (!lds) {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_BUILD);
        HIP_TRY(hipMemsetAsync(d_flag, 0, 4, c->stream));
        HIP_TRY(hipMemsetAsync(d_table, 0xFF, (size_t)slots * 8, c->stream));
        if (n_values) {
            const int bgrid = (int)std::min<int64_t>((int64_t)c->n_cu * 8, (n_values + PRED_THREADS - 1) / PRED_THREADS);
            hipLaunchKernelGGL(pred_isin_build_kernel, dim3(bgrid), dim3(PRED_THREADS), 0, c->stream, ps);
        }
        HIP_TRY(hipGetLastError());
    }
    {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_PROBE);
        if (key == 0) ST_TRY(pred_launch_isin<0>(c, lds, grid, pc, tiles, ps, negate ? 1 : 0, po));
        else if (key == 1) ST_TRY(pred_launch_isin<1>(c, lds, grid, pc, tiles, ps, negate ? 1 : 0, po));
        else ST_TRY(pred_launch_isin<2>(c, lds, grid, pc, tiles, ps, negate ? 1 : 0, po));
        HIP_TRY(hipGetLastError());
    }
    c->timings.table_slots = slots;
    c->timings.n_partitions = lds ? 1 : 2;              // which set answered: 1 = LDS, 2 = global
    c->timings.algorithmic_bytes = (int64_t)dtype_bytes(col->dtype, n_rows) + (cv.mask ? (int64_t)nbytes : 0) + (d_bits ? (int64_t)nbytes : 0) +
                                   (int64_t)vbytes;
    PredCall call{c, nbytes, out_bits, out_count};
    return call.finish(stg, d_count);
}

}  // namespace pandrs
