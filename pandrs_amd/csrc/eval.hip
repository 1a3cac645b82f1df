// eval.hip — derived columns: one postfix program over up to eight columns, evaluated per row in one stream, behind
// PandasCompatExt::add_scalar .. sqrt (reference src/dataframe/pandas_compat/functions.rs:2819-2840), col_add .. col_div
// (:2851-2960), add_columns .. div_columns (:3890-3984), coalesce (:3846), clip (:237), where_cond / mask (:1079-1139), sign
// (:3998-4014), normalize (:2316-2337) and helpers/math_ops.rs, gfx950, wave64.
//
// The program is postfix over a typed stack of values (f64) and booleans.  Where every entry of a postfix program sits on the stack
// is known before it runs, so the host validates the program and lowers it to three-address code: instruction i is (op, d), reads
// the slots d, d + 1 (d + 2: SELECT) and writes slot d; a CONST or COL pushed right before a two-operand op is folded into it
// (x + 1.5 is two instructions, a * b + c three).  The kernel gets the lowered program by value in its arguments: every lane runs
// the same instruction, the dispatch is scalar and uniform, and the eight slots are named registers picked in a uniform switch:
// no array is indexed by a run-time value, so nothing goes to scratch.  A boolean lives in a slot as 1.0 / 0.0.
// Rows: a wave owns 128 consecutive rows per step, lane l the rows 2 l and 2 l + 1: 16-byte loads and stores for 8-byte cells (two
// 8-byte accesses for a buffer that is only 8-byte aligned, the same lines either way).  Every distinct column the program names is
// loaded once per row, the program runs out of registers, the result leaves with one store.  Three instantiations by the columns
// and slots a program needs keep four, two or one steps of loads in flight per wave: registers bound the loads in flight.  Bits
// (a boolean result, the null mask of a value result) leave as two wave ballots woven into the 128-row word, stored bytewise by
// lanes 0 .. 15.
#include "engine.hpp"

#include <algorithm>
#include <cmath>

namespace pandrs {

#pragma clang fp contract(off)      // every operation is rounded on its own: a * b + c is two roundings, as in the reference

constexpr int EVAL_THREADS = 256;                       // 4 waves
constexpr int EVAL_WAVES = EVAL_THREADS / 64;
constexpr int EVAL_STEPS = 4;                           // steps of 128 rows per wave and tile
constexpr int EVAL_TILE = EVAL_WAVES * EVAL_STEPS * 128;        // 2048 rows: eval_tile_rows of pandrs_hip.h
constexpr int EVAL_BLOCKS_PER_CU = 4;                   // eval_blocks_per_cu of pandrs_hip.h
constexpr int EVAL_MAX_OPS = 64, EVAL_MAX_COLS = 8, EVAL_MAX_DEPTH = 8;

struct EvalProg {                   // the lowered program
    double cst[EVAL_MAX_OPS];       // CONST: the constant
    uint8_t op[EVAL_MAX_OPS];       // pandrs_hip_eval_op
    uint8_t dst[EVAL_MAX_OPS];      // the slot written; the operands are dst, dst + 1, dst + 2
    uint8_t col[EVAL_MAX_OPS];      // COL, or a folded column operand: the column's number
    uint8_t bk[EVAL_MAX_OPS];       // where the second operand comes from: 0 slot dst + 1, 1 cst (a folded CONST), 2 col (a folded COL)
    int32_t n_ops;                  // instructions after folding
    int32_t n_cols;                 // the named columns, numbered 0 .. n_cols - 1 in the order of first use
    uint32_t used;                  // host: bit c, a COL names the caller's column c
    uint8_t number[EVAL_MAX_COLS];  // host: the number of the caller's column c
    int32_t depth;                  // host: the slots the instructions touch
};

struct EvalCols {
    const void *data[EVAL_MAX_COLS];
    const uint8_t *mask[EVAL_MAX_COLS];     // null bits or nullptr
    uint8_t dtype[EVAL_MAX_COLS];
    uint8_t in16[EVAL_MAX_COLS];            // data is 16-byte aligned
    int64_t n;
};

struct EvalOut {
    uint64_t *data;                 // a value program: n cells
    uint8_t *bits;                  // a value program: the null mask or nullptr; a boolean program: the bitmap
    unsigned long long *count;      // += the bits set
    int out16;                      // data is 16-byte aligned
};

__device__ __forceinline__ double eval_nan() { return __longlong_as_double((long long)CANON_NAN); }

// the 128-row word that starts at row0: b0 holds the rows 2 l, b1 the rows 2 l + 1.  Lane j < 16 owns byte j = the lanes 4 j .. 4 j + 3;
// no byte at or past ceil(n / 8) is touched (rows past n never set a bit, so the last byte's high bits are 0).
__device__ __forceinline__ void eval_store_bits(uint8_t *bits, int64_t row0, int64_t n, uint64_t b0, uint64_t b1, uint32_t lane) {
    const int64_t byte = (row0 >> 3) + lane;
    if (lane < 16 && byte < ((n + 7) >> 3)) {
        const uint32_t e = (uint32_t)(b0 >> (lane * 4)) & 0xFu, o = (uint32_t)(b1 >> (lane * 4)) & 0xFu;
        const uint32_t se = (e & 1u) | (e & 2u) << 1 | (e & 4u) << 2 | (e & 8u) << 3;
        const uint32_t so = (o & 1u) | (o & 2u) << 1 | (o & 4u) << 2 | (o & 8u) << 3;
        bits[byte] = (uint8_t)(se | so << 1);
    }
}

// Slots and columns are named scalars, and the uniform slot number picks among them in a switch with one literal name per case (an
// array picked by a run-time index, even through an unrolled loop of selects, goes to scratch at eight entries).
#define EVAL_GET(K) case K: if (K < ND) { ax = s##K##x; ay = s##K##y; } if (K + 1 < ND) { bx = EVAL_NEXT(K, x); by = EVAL_NEXT(K, y); } break;
#define EVAL_NEXT(K, F) (K == 0 ? s1##F : K == 1 ? s2##F : K == 2 ? s3##F : K == 3 ? s4##F : K == 4 ? s5##F : K == 5 ? s6##F : s7##F)
#define EVAL_GET2(K) case K: if (K + 2 < ND) { ex = EVAL_NEXT2(K, x); ey = EVAL_NEXT2(K, y); } break;
#define EVAL_NEXT2(K, F) (K == 0 ? s2##F : K == 1 ? s3##F : K == 2 ? s4##F : K == 3 ? s5##F : K == 4 ? s6##F : s7##F)
#define EVAL_COLGET(J, X, Y) case J: if (J < NC) { X = v##J##x; Y = v##J##y; } break;
#define EVAL_PUT(K) case K: if (K < ND) { s##K##x = rx; s##K##y = ry; } break;

// NC: the columns a program of this instantiation may name (the host numbers the named columns 0 .. n_cols - 1), ND: its stack
// slots, U: the steps whose loads are in flight together.  Fewer registers for the small programs mean more waves per SIMD.
template <bool IS_MASK, int NC, int ND, int U>
__global__ __launch_bounds__(EVAL_THREADS) void eval_kernel(EvalCols c, EvalProg p, int64_t tiles, EvalOut o) {
    static_assert(EVAL_STEPS % U == 0, "the steps of a tile come in groups of U");
    __shared__ uint32_t s_cnt[EVAL_WAVES];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    uint32_t set = 0;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        for (int k0 = 0; k0 < EVAL_STEPS; k0 += U) {    // (uniform loops: the ballots see every lane)
            // ---- pass 1: every load of these U steps is in flight before the first cell is looked at ----
            uint64_t qa[U][NC], qb[U][NC];
            uint32_t qm[U][NC];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int64_t r0 = t * EVAL_TILE + (int64_t)((k0 + u) * EVAL_WAVES + wave) * 128 + 2 * lane;
                const bool in0 = r0 < c.n, in1 = r0 + 1 < c.n;
#pragma unroll
                for (int j = 0; j < NC; j++) {
                    qa[u][j] = qb[u][j] = 0;
                    qm[u][j] = 0;
                    if (j < p.n_cols) {
                        if (c.mask[j] && in0) qm[u][j] = c.mask[j][r0 >> 3];                    // r0 is even: both bits in one byte
                        if (c.dtype[j] == PANDRS_HIP_BOOLBITS) {
                            if (in0) qa[u][j] = static_cast<const uint8_t *>(c.data[j])[r0 >> 3];
                        } else {
                            const uint64_t *d = static_cast<const uint64_t *>(c.data[j]);
                            if (in1 && c.in16[j]) {
                                const ulonglong2 q = *reinterpret_cast<const ulonglong2 *>(d + r0);
                                qa[u][j] = q.x; qb[u][j] = q.y;
                            } else {
                                if (in0) qa[u][j] = d[r0];
                                if (in1) qb[u][j] = d[r0 + 1];
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int64_t row0 = t * EVAL_TILE + (int64_t)((k0 + u) * EVAL_WAVES + wave) * 128, r0 = row0 + 2 * lane;
                if (row0 >= c.n) continue;              // (uniform: the whole wave)
                const bool in0 = r0 < c.n, in1 = r0 + 1 < c.n;
                // ---- pass 2: a numeric cell as f64 (NaN under a null bit), a boolean as 1.0 / 0.0 (0.0 under one) ----
                double v0x = 0, v0y = 0, v1x = 0, v1y = 0, v2x = 0, v2y = 0, v3x = 0, v3y = 0, v4x = 0, v4y = 0, v5x = 0, v5y = 0, v6x = 0, v6y = 0, v7x = 0, v7y = 0;
                uint32_t nulls = 0;                     // bit 0 / 1: a named cell of row r0 / r0 + 1 is null
#define EVAL_CELL(J)                                                                                                             \
                if (J < NC && J < p.n_cols) {                                                                                    \
                    const int j = J < NC ? J : 0;                                                                                \
                    const uint32_t nb = (qm[u][j] >> (r0 & 7)) & (in1 ? 3u : 1u);                                                \
                    if (c.dtype[j] == PANDRS_HIP_BOOLBITS) {                                                                     \
                        const uint32_t b = ((uint32_t)qa[u][j] >> (r0 & 7)) & 3u & ~nb;                                          \
                        v##J##x = (b & 1) ? 1.0 : 0.0;                                                                           \
                        v##J##y = (b & 2) ? 1.0 : 0.0;                                                                           \
                    } else {                                                                                                     \
                        const bool i64 = c.dtype[j] == PANDRS_HIP_I64;                                                           \
                        v##J##x = (nb & 1) ? eval_nan() : i64 ? (double)(int64_t)qa[u][j] : __longlong_as_double((long long)qa[u][j]); \
                        v##J##y = (nb & 2) ? eval_nan() : i64 ? (double)(int64_t)qb[u][j] : __longlong_as_double((long long)qb[u][j]); \
                    }                                                                                                            \
                    nulls |= nb;                                                                                                 \
                }
                EVAL_CELL(0) EVAL_CELL(1) EVAL_CELL(2) EVAL_CELL(3) EVAL_CELL(4) EVAL_CELL(5) EVAL_CELL(6) EVAL_CELL(7)
#undef EVAL_CELL
                // ---- the program: instruction i reads the slots d, d + 1 (d + 2) and writes slot d ----
                double s0x = 0, s0y = 0, s1x = 0, s1y = 0, s2x = 0, s2y = 0, s3x = 0, s3y = 0, s4x = 0, s4y = 0, s5x = 0, s5y = 0, s6x = 0, s6y = 0, s7x = 0, s7y = 0;
                for (int i = 0; i < p.n_ops; i++) {     // (uniform: p lives in the kernel arguments)
                    const int op = p.op[i], d = p.dst[i];
                    double rx = 0.0, ry = 0.0;
                    if (op == PANDRS_HIP_EVAL_COL) {
                        switch (p.col[i]) {
                        EVAL_COLGET(0, rx, ry) EVAL_COLGET(1, rx, ry) EVAL_COLGET(2, rx, ry) EVAL_COLGET(3, rx, ry)
                        EVAL_COLGET(4, rx, ry) EVAL_COLGET(5, rx, ry) EVAL_COLGET(6, rx, ry) EVAL_COLGET(7, rx, ry)
                        }
                    } else if (op == PANDRS_HIP_EVAL_CONST) {
                        rx = ry = p.cst[i];
                    } else {
                        double ax = 0.0, ay = 0.0, bx = 0.0, by = 0.0;
                        switch (d) {                    // the first operand, and the slot above it (read by the ops with two operands only)
                        EVAL_GET(0) EVAL_GET(1) EVAL_GET(2) EVAL_GET(3) EVAL_GET(4) EVAL_GET(5) EVAL_GET(6) EVAL_GET(7)
                        }
                        const int bk = p.bk[i];         // a CONST or COL pushed right before a two-operand op was folded into it by the host
                        if (bk == 1) {
                            bx = by = p.cst[i];
                        } else if (bk == 2) {
                            switch (p.col[i]) {
                            EVAL_COLGET(0, bx, by) EVAL_COLGET(1, bx, by) EVAL_COLGET(2, bx, by) EVAL_COLGET(3, bx, by)
                            EVAL_COLGET(4, bx, by) EVAL_COLGET(5, bx, by) EVAL_COLGET(6, bx, by) EVAL_COLGET(7, bx, by)
                            }
                        }
                        switch (op) {
                        case PANDRS_HIP_EVAL_ADD: rx = ax + bx; ry = ay + by; break;
                        case PANDRS_HIP_EVAL_SUB: rx = ax - bx; ry = ay - by; break;
                        case PANDRS_HIP_EVAL_MUL: rx = ax * bx; ry = ay * by; break;
                        case PANDRS_HIP_EVAL_DIV: rx = ax / bx; ry = ay / by; break;
                        case PANDRS_HIP_EVAL_REM: rx = fmod(ax, bx); ry = fmod(ay, by); break;
                        case PANDRS_HIP_EVAL_MAX: rx = fmax(ax, bx); ry = fmax(ay, by); break;
                        case PANDRS_HIP_EVAL_MIN: rx = fmin(ax, bx); ry = fmin(ay, by); break;
                        case PANDRS_HIP_EVAL_NEG: rx = -ax; ry = -ay; break;
                        case PANDRS_HIP_EVAL_ABS: rx = fabs(ax); ry = fabs(ay); break;
                        case PANDRS_HIP_EVAL_FLOOR: rx = floor(ax); ry = floor(ay); break;
                        case PANDRS_HIP_EVAL_CEIL: rx = ceil(ax); ry = ceil(ay); break;
                        case PANDRS_HIP_EVAL_TRUNC: rx = trunc(ax); ry = trunc(ay); break;
                        case PANDRS_HIP_EVAL_ROUND: rx = round(ax); ry = round(ay); break;
                        case PANDRS_HIP_EVAL_FRACT: rx = ax - trunc(ax); ry = ay - trunc(ay); break;
                        case PANDRS_HIP_EVAL_SQRT: rx = sqrt(ax); ry = sqrt(ay); break;
                        case PANDRS_HIP_EVAL_SIGN:      // functions.rs:3998-4014: NaN and both zeros give 0
                            rx = ax > 0.0 ? 1.0 : ax < 0.0 ? -1.0 : 0.0;
                            ry = ay > 0.0 ? 1.0 : ay < 0.0 ? -1.0 : 0.0;
                            break;
                        case PANDRS_HIP_EVAL_GT: rx = ax > bx ? 1.0 : 0.0; ry = ay > by ? 1.0 : 0.0; break;
                        case PANDRS_HIP_EVAL_GE: rx = ax >= bx ? 1.0 : 0.0; ry = ay >= by ? 1.0 : 0.0; break;
                        case PANDRS_HIP_EVAL_LT: rx = ax < bx ? 1.0 : 0.0; ry = ay < by ? 1.0 : 0.0; break;
                        case PANDRS_HIP_EVAL_LE: rx = ax <= bx ? 1.0 : 0.0; ry = ay <= by ? 1.0 : 0.0; break;
                        case PANDRS_HIP_EVAL_EQ: rx = ax == bx ? 1.0 : 0.0; ry = ay == by ? 1.0 : 0.0; break;
                        case PANDRS_HIP_EVAL_NE: rx = ax != bx ? 1.0 : 0.0; ry = ay != by ? 1.0 : 0.0; break;
                        case PANDRS_HIP_EVAL_ISNAN: rx = ax != ax ? 1.0 : 0.0; ry = ay != ay ? 1.0 : 0.0; break;
                        case PANDRS_HIP_EVAL_ISINF: rx = fabs(ax) == INFINITY ? 1.0 : 0.0; ry = fabs(ay) == INFINITY ? 1.0 : 0.0; break;
                        case PANDRS_HIP_EVAL_ISFINITE: rx = fabs(ax) < INFINITY ? 1.0 : 0.0; ry = fabs(ay) < INFINITY ? 1.0 : 0.0; break;
                        case PANDRS_HIP_EVAL_AND: rx = ax != 0.0 && bx != 0.0 ? 1.0 : 0.0; ry = ay != 0.0 && by != 0.0 ? 1.0 : 0.0; break;
                        case PANDRS_HIP_EVAL_OR: rx = ax != 0.0 || bx != 0.0 ? 1.0 : 0.0; ry = ay != 0.0 || by != 0.0 ? 1.0 : 0.0; break;
                        case PANDRS_HIP_EVAL_NOT: rx = ax != 0.0 ? 0.0 : 1.0; ry = ay != 0.0 ? 0.0 : 1.0; break;
                        default: {                      // SELECT: cond in d, a in d + 1, b in d + 2
                            double ex = 0.0, ey = 0.0;
                            switch (d) {
                            EVAL_GET2(0) EVAL_GET2(1) EVAL_GET2(2) EVAL_GET2(3) EVAL_GET2(4) EVAL_GET2(5)
                            }
                            rx = ax != 0.0 ? bx : ex;
                            ry = ay != 0.0 ? by : ey;
                        }
                        }
                    }
                    switch (d) {                        // (a literal index per case: a loop over the slots becomes one indexed store)
                    EVAL_PUT(0) EVAL_PUT(1) EVAL_PUT(2) EVAL_PUT(3) EVAL_PUT(4) EVAL_PUT(5) EVAL_PUT(6) EVAL_PUT(7)
                    }
                }
                // ---- the result: slot 0 ----
                if (IS_MASK) {
                    const uint64_t b0 = __ballot(in0 && s0x != 0.0), b1 = __ballot(in1 && s0y != 0.0);
                    if (o.bits) eval_store_bits(o.bits, row0, c.n, b0, b1, lane);
                    if (lane == 0) set += (uint32_t)(__popcll(b0) + __popcll(b1));
                } else {
                    const bool n0 = s0x != s0x, n1 = s0y != s0y;
                    ulonglong2 q;                       // every NaN leaves as the canonical one
                    q.x = n0 ? CANON_NAN : (uint64_t)__double_as_longlong(s0x);
                    q.y = n1 ? CANON_NAN : (uint64_t)__double_as_longlong(s0y);
                    if (in1 && o.out16) {
                        *reinterpret_cast<ulonglong2 *>(o.data + r0) = q;
                    } else {
                        if (in0) o.data[r0] = q.x;
                        if (in1) o.data[r0 + 1] = q.y;
                    }
                    const uint64_t b0 = __ballot(in0 && n0 && (nulls & 1)), b1 = __ballot(in1 && n1 && (nulls & 2));
                    if (o.bits) eval_store_bits(o.bits, row0, c.n, b0, b1, lane);
                    if (lane == 0) set += (uint32_t)(__popcll(b0) + __popcll(b1));
                }
            }
        }
    }
    if (lane == 0) s_cnt[wave] = set;                   // the waves' counts -> one atomic add per workgroup
    __syncthreads();
    if (tid == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < EVAL_WAVES; w++) s += s_cnt[w];
        if (s) atomicAdd(o.count, s);
    }
}

#undef EVAL_GET
#undef EVAL_NEXT
#undef EVAL_GET2
#undef EVAL_NEXT2
#undef EVAL_COLGET
#undef EVAL_PUT

// ---- host -------------------------------------------------------------------------------------------------------------------------
// The validator and the lowering in one walk: a stack of types, the slot every op writes.  Needs no context and no device.
static int32_t eval_lower(const int32_t *col_dtypes, int32_t n_cols, const int32_t *ops, const double *args, int32_t n_ops, EvalProg *prog,
                          int32_t *out_is_mask, int32_t *out_depth) {
    if (!col_dtypes || !ops || !args) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "eval: bad arguments");
    if (n_cols < 1 || n_cols > EVAL_MAX_COLS)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "eval: %d columns; a program reads 1 .. %d", n_cols, EVAL_MAX_COLS);
    if (n_ops < 1 || n_ops > EVAL_MAX_OPS)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "eval: %d ops; a program has 1 .. %d", n_ops, EVAL_MAX_OPS);
    bool is_bool[EVAL_MAX_DEPTH] = {};
    int sp = 0, depth = 0;
    if (prog) *prog = EvalProg{};
    for (int i = 0; i < n_ops; i++) {
        const int op = ops[i];
        if (op < PANDRS_HIP_EVAL_COL || op > PANDRS_HIP_EVAL_SELECT)
            return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "eval: op %d: %d is not a pandrs_hip_eval_op", i, op);
        int pops, col = 0;
        bool out_bool = false;
        if (op <= PANDRS_HIP_EVAL_CONST) pops = 0;
        else if (op <= PANDRS_HIP_EVAL_MIN) pops = 2;
        else if (op <= PANDRS_HIP_EVAL_SIGN) pops = 1;
        else if (op <= PANDRS_HIP_EVAL_NE) pops = 2;
        else if (op <= PANDRS_HIP_EVAL_ISFINITE) pops = 1;
        else if (op <= PANDRS_HIP_EVAL_OR) pops = 2;
        else if (op == PANDRS_HIP_EVAL_NOT) pops = 1;
        else pops = 3;
        if (sp < pops) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "eval: op %d: the stack holds %d entries, the op takes %d", i, sp, pops);
        const bool *top = is_bool + sp - pops;          // the operands in push order
        if (op == PANDRS_HIP_EVAL_COL) {
            const double a = args[i];
            if (!(a >= 0.0 && a < (double)n_cols) || a != std::floor(a))
                return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "eval: op %d: %g is not a column index in [0, %d)", i, a, n_cols);
            col = (int)a;
            const int dt = col_dtypes[col];
            if (dt != PANDRS_HIP_I64 && dt != PANDRS_HIP_F64 && dt != PANDRS_HIP_BOOLBITS)
                return fail(PANDRS_HIP_ERR_TYPE_MISMATCH, "eval: op %d: column %d has dtype %d, expected I64, F64 or BOOLBITS", i, col, dt);
            out_bool = dt == PANDRS_HIP_BOOLBITS;
        } else if (op >= PANDRS_HIP_EVAL_AND && op <= PANDRS_HIP_EVAL_NOT) {
            for (int k = 0; k < pops; k++)
                if (!top[k]) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "eval: op %d: operand %d is a value, the op takes booleans", i, k);
            out_bool = true;
        } else if (op == PANDRS_HIP_EVAL_SELECT) {
            if (!top[0]) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "eval: op %d: the condition of SELECT is a value", i);
            if (top[1] != top[2]) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "eval: op %d: the branches of SELECT differ in type", i);
            out_bool = top[1];
        } else if (op != PANDRS_HIP_EVAL_CONST) {
            for (int k = 0; k < pops; k++)
                if (top[k]) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "eval: op %d: operand %d is a boolean, the op takes values", i, k);
            out_bool = op >= PANDRS_HIP_EVAL_GT;
        }
        sp -= pops;
        if (sp >= EVAL_MAX_DEPTH) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "eval: op %d: the stack would hold more than %d entries", i, EVAL_MAX_DEPTH);
        if (prog) {
            if (op == PANDRS_HIP_EVAL_COL && !(prog->used >> col & 1)) {
                prog->used |= 1u << col;
                prog->number[col] = (uint8_t)prog->n_cols++;
            }
            int k = prog->n_ops;                        // the instruction: (op, slot sp); its operands sit in the slots sp, sp + 1, sp + 2
            const bool takes_values = pops == 2 && op != PANDRS_HIP_EVAL_AND && op != PANDRS_HIP_EVAL_OR;
            if (takes_values && k > 0 && prog->dst[k - 1] == sp + 1 && prog->bk[k - 1] == 0 &&
                (prog->op[k - 1] == PANDRS_HIP_EVAL_CONST || prog->op[k - 1] == PANDRS_HIP_EVAL_COL)) {
                k--;                                    // the push right before it made its second operand: folded into the op
                prog->bk[k] = prog->op[k] == PANDRS_HIP_EVAL_CONST ? 1 : 2;
            } else {
                prog->bk[k] = 0;
                prog->col[k] = op == PANDRS_HIP_EVAL_COL ? prog->number[col] : 0;
                prog->cst[k] = op == PANDRS_HIP_EVAL_CONST ? args[i] : 0.0;
            }
            prog->op[k] = (uint8_t)op;
            prog->dst[k] = (uint8_t)sp;
            prog->n_ops = k + 1;
        }
        is_bool[sp++] = out_bool;
        depth = std::max(depth, sp);
    }
    if (sp != 1) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "eval: op %d: the program leaves %d entries on the stack, expected 1", n_ops - 1, sp);
    if (prog) {                                         // the slots the instructions touch: fewer than the postfix depth after folding
        prog->depth = 1;
        for (int k = 0; k < prog->n_ops; k++) {
            const int reach = prog->op[k] == PANDRS_HIP_EVAL_SELECT ? 3 : prog->bk[k] == 0 && prog->op[k] >= PANDRS_HIP_EVAL_ADD ? 2 : 1;
            prog->depth = std::max<int32_t>(prog->depth, prog->dst[k] + reach);
        }
        prog->depth = std::min<int32_t>(prog->depth, EVAL_MAX_DEPTH);
    }
    if (out_is_mask) *out_is_mask = is_bool[0] ? 1 : 0;
    if (out_depth) *out_depth = depth;
    return 0;
}

int32_t eval_check_entry(const int32_t *col_dtypes, int32_t n_cols, const int32_t *ops, const double *args, int32_t n_ops, int32_t *out_is_mask,
                         int32_t *out_depth) {
    return eval_lower(col_dtypes, n_cols, ops, args, n_ops, nullptr, out_is_mask, out_depth);
}

static bool eval_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && na && nb && x < y + nb && y < x + na;
}

// the instantiation by what the program needs: few columns and a shallow stack leave registers for more loads in flight
template <bool IS_MASK>
static void eval_launch(pandrs_hip_ctx *c, int grid, const EvalCols &ec, const EvalProg &prog, int64_t tiles, const EvalOut &eo) {
    if (prog.n_cols <= 2 && prog.depth <= 4)
        hipLaunchKernelGGL((eval_kernel<IS_MASK, 2, 4, 4>), dim3(grid), dim3(EVAL_THREADS), 0, c->stream, ec, prog, tiles, eo);
    else if (prog.n_cols <= 4)
        hipLaunchKernelGGL((eval_kernel<IS_MASK, 4, EVAL_MAX_DEPTH, 2>), dim3(grid), dim3(EVAL_THREADS), 0, c->stream, ec, prog, tiles, eo);
    else
        hipLaunchKernelGGL((eval_kernel<IS_MASK, EVAL_MAX_COLS, EVAL_MAX_DEPTH, 1>), dim3(grid), dim3(EVAL_THREADS), 0, c->stream, ec, prog, tiles, eo);
}

int32_t eval_entry(pandrs_hip_ctx *c, int32_t mem_space, const pandrs_hip_column *cols, int32_t n_cols, int64_t n_rows, const int32_t *ops,
                   const double *args, int32_t n_ops, int32_t out_mem_space, void *out_data, uint8_t *out_null_mask, int64_t *out_count) {
    if (!c || !cols || n_rows < 0) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "eval: bad arguments");
    ST_TRY(check_mem_space("eval", mem_space, out_mem_space));
    int32_t dtypes[EVAL_MAX_COLS] = {};
    for (int j = 0; j < std::min(n_cols, (int32_t)EVAL_MAX_COLS); j++) dtypes[j] = cols[j].dtype;
    EvalProg prog;
    int32_t is_mask = 0;
    ST_TRY(eval_lower(dtypes, n_cols, ops, args, n_ops, &prog, &is_mask, nullptr));
    if (is_mask && out_null_mask) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "eval: a boolean program takes no out_null_mask");
    if (is_mask ? (!out_data && !out_count) : (n_rows > 0 && !out_data)) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "eval: no output");
    if (n_rows >= (int64_t(1) << 32))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "eval: %lld rows; one call takes fewer than 2^32", (long long)n_rows);
    for (int j = 0; j < n_cols; j++)
        if ((prog.used >> j & 1) && n_rows > 0 && !cols[j].data) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "eval: column %d has no data", j);
    if (out_count) *out_count = 0;
    if (n_rows == 0) return 0;
    const size_t n = (size_t)n_rows, nbytes = (n + 7) / 8, out_bytes = is_mask ? nbytes : n * 8;
    if (mem_space == out_mem_space)
        for (int j = 0; j < n_cols; j++) {
            if (!(prog.used >> j & 1)) continue;
            const size_t cb = dtype_bytes(cols[j].dtype, n_rows);
            for (const void *out : {(const void *)out_data, (const void *)out_null_mask})
                if (eval_overlap(out, out == out_data ? out_bytes : nbytes, cols[j].data, cb) ||
                    eval_overlap(out, out == out_data ? out_bytes : nbytes, cols[j].null_mask, nbytes))
                    return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "eval: an output overlaps column %d; the call cannot run in place", j);
        }
    std::lock_guard<std::mutex> lock(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    timings_begin(c);

    // ---- staging: the named host columns, a host out_data, a host out_null_mask (its own slot), sized up front ----
    ColView cv[EVAL_MAX_COLS] = {};
    void *d_out = out_data;
    uint8_t *d_omask = out_null_mask;
    Stager stg{c, mem_space, out_mem_space};
    const bool stage_mask = out_null_mask && out_mem_space == PANDRS_HIP_MEM_HOST;
    size_t need = stg.out_size(out_data, out_bytes) + (stage_mask ? Stager::slot(nbytes) : 0);
    for (int j = 0; j < n_cols; j++) {
        cv[j] = ColView{cols[j].data, cols[j].null_mask};
        if (prog.used >> j & 1) need += stg.col_size(cols[j], n_rows);
    }
    if (need) {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_STAGE_IN);
        ST_TRY(stg.reserve(need));
        for (int j = 0; j < n_cols; j++)
            if (prog.used >> j & 1) cv[j] = stg.col(cols[j], n_rows);
        d_out = stg.out(out_data, out_bytes);
        if (stage_mask) d_omask = stg.scratch<uint8_t>(nbytes);
        if (stg.status) return stg.status;
    }
    EvalCols ec{};
    ec.n = n_rows;
    int64_t in_bytes = 0;
    for (int j = 0; j < n_cols; j++) {
        if (!(prog.used >> j & 1)) continue;
        const bool bits = cols[j].dtype == PANDRS_HIP_BOOLBITS;
        if (!bits && (reinterpret_cast<uintptr_t>(cv[j].data) & 7))
            return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "eval: column %d must be 8-byte aligned", j);
        const int k = prog.number[j];
        ec.data[k] = cv[j].data;
        ec.mask[k] = cv[j].mask;
        ec.dtype[k] = (uint8_t)cols[j].dtype;
        ec.in16[k] = (reinterpret_cast<uintptr_t>(cv[j].data) & 15) == 0;
        in_bytes += (int64_t)dtype_bytes(cols[j].dtype, n_rows) + (cv[j].mask ? (int64_t)nbytes : 0);
    }
    if (!is_mask && (reinterpret_cast<uintptr_t>(d_out) & 7)) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "eval: out_data must be 8-byte aligned");
    ST_TRY(c->work.ensure(Arena::padded(8), c->stream));
    unsigned long long *d_count = c->work.take<unsigned long long>(1);
    if (!d_count) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (eval)");

    const int64_t tiles = (n_rows + EVAL_TILE - 1) / EVAL_TILE;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)c->n_cu * EVAL_BLOCKS_PER_CU, tiles));
    EvalOut eo{is_mask ? nullptr : static_cast<uint64_t *>(d_out), is_mask ? static_cast<uint8_t *>(d_out) : d_omask, d_count,
               (reinterpret_cast<uintptr_t>(d_out) & 15) == 0};
    {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_AGGREGATE);
        HIP_TRY(hipMemsetAsync(d_count, 0, 8, c->stream));
        if (is_mask) eval_launch<true>(c, grid, ec, prog, tiles, eo);
        else eval_launch<false>(c, grid, ec, prog, tiles, eo);
        HIP_TRY(hipGetLastError());
    }
    // every named column and its mask read once, the result (and its mask) written once
    c->timings.algorithmic_bytes = in_bytes + (d_out ? (int64_t)out_bytes : 0) + (!is_mask && d_omask ? (int64_t)nbytes : 0);
    ST_TRY(stg.copy_back(out_bytes));
    if (stage_mask) HIP_TRY(hipMemcpyAsync(out_null_mask, d_omask, nbytes, hipMemcpyDeviceToHost, c->stream));
    unsigned long long count = 0;
    HIP_TRY(hipMemcpyAsync(&count, d_count, 8, hipMemcpyDeviceToHost, c->stream));
    ST_TRY(timings_end(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (out_count) *out_count = (int64_t)count;
    return 0;
}

}  // namespace pandrs
