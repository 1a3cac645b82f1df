// pivot.hip — a group-by over two key columns laid out as a dense matrix, behind crosstab (reference
// src/dataframe/pandas_compat/functions.rs:2138-2183), pivot_table (src/pivot/mod.rs:12-250) and pivot / unstack
// (functions.rs:2471-2527), gfx950, wave64.  pandrs_hip.h states the contract: the labels of either key column are its distinct
// numbers in pandrs_hip_distinct's BY_VALUE order, then at most one missing label (NaN and null cells together); the cells are
// column-major [j * R + i]; rows per cell are exact int64; a cell's value is what the engine's aggregate gives for its group.
// 1. Census: distinct.hpp's census over either key column (two launches, one read-back): min, max, the missing counts, F64
//    integrality and -0.0 presence.
// 2. Direct path, when both columns are addressable by value and (cells1 + 1) x (cells2 + 1) <= PV_DIRECT_MAX_CELLS: ONE stream
//    reads the two keys and the value of every row and accumulates into a per-workgroup table in LDS, in span coordinates (the
//    number's distance from the column's smallest one; the last slot of either dimension is the missing label).  Lanes of a
//    wave holding the same cell combine by ballot and a wave reduction before they touch LDS, the rest use LDS atomics.  A
//    workgroup folds its non-empty cells into the 64-bit workspace table when it ends.  One small workgroup then drops span rows
//    and span columns without a row, orders the labels and writes the dense result.  No workgroup waits for another.
// 3. General path, everything else: the groupby engine lists either column's distinct cells (COUNT), the radix sort orders them
//    into the label lists, the engine runs over the two key columns with the op and COUNT, and a small kernel looks either key
//    cell of every GROUP up in the sorted label lists and writes the group into its dense cell.
#include "distinct.hpp"

#include <algorithm>

namespace pandrs {

constexpr int PV_THREADS = 256;
constexpr int PV_LOADS = 4;                              // 16-byte loads in flight per thread and column
constexpr int PV_TILE = PV_THREADS * PV_LOADS * 2;       // rows per workgroup iteration (2048; pandrs_hip.h: pivot_tile_rows)
constexpr int PV_BLOCKS_PER_CU = 4;                      // pandrs_hip.h: pivot_blocks_per_cu
constexpr int PV_DIRECT_MAX_CELLS = 4096;                // pandrs_hip.h: pivot_direct_max_cells; at most 16 bytes of LDS per cell: 64 KiB per workgroup
constexpr int64_t PV_MAX_CELLS = 16777216;               // pandrs_hip.h: pivot_max_cells; 16 bytes per retained cell: 256 MiB
constexpr int PV_PEEL = 4;                               // cells a wave folds by ballot before plain atomics
constexpr int PV_PEEL_MIN = 4;                           // ... as long as a round folds at least this many lanes
constexpr int PV_FINISH_THREADS = 256;

// what the stream keeps per cell beside the row count
enum { PV_CLS_ROWS = 0,      // ROWS, COUNT: nothing
       PV_CLS_SUM_F64,       // SUM, MEAN of an F64 column: an f64 sum and the non-null cells
       PV_CLS_SUM_I64,       // SUM, MEAN of an I64 column: a wrapping int64 sum and the non-null cells
       PV_CLS_EXTREME,       // MIN, MAX: the order image of the extreme
       PV_CLS_LAST };        // LAST: the largest row index

struct PvArgs {
    DnCol k1, k2, v;          // v.data == nullptr: no value column
    int32_t dt1, dt2;
    int32_t v_i64, is_max;    // the value column holds I64; MAX instead of MIN
    uint64_t base1, base2;
    uint32_t n1, n2;          // value slots of either dimension; slot n1 / n2 is the missing label
    uint64_t init;            // what an untouched state cell holds
    unsigned long long *g_rows, *g_state, *g_nn;      // (n1 + 1) * (n2 + 1) cells each, column-major
};

__device__ __forceinline__ void pv_load_key(int dt, const DnCol &c, int64_t r, bool aligned, uint64_t v[2], uint32_t &in) {
    switch (dt) {
    case PANDRS_HIP_I64: case PANDRS_HIP_F64: dn_load2<PANDRS_HIP_I64>(c, r, aligned, v, in); break;
    case PANDRS_HIP_U32CODE: dn_load2<PANDRS_HIP_U32CODE>(c, r, aligned, v, in); break;
    default: dn_load2<PANDRS_HIP_BOOLBITS>(c, r, aligned, v, in); break;
    }
}

// the slot of a key cell in its dimension: n (the missing label) for a null or NaN cell
__device__ __forceinline__ uint32_t pv_slot(int dt, uint64_t cell, bool null, uint64_t base, uint32_t n, bool &ok) {
    if (null || (dt == PANDRS_HIP_F64 && dn_is_nan(cell))) return n;
    const uint64_t idx = dt == PANDRS_HIP_F64 ? dn_cell_index<PANDRS_HIP_F64>(cell, base) : cell - base;
    ok = ok && idx < (uint64_t)n;                        // (the census bounds every number: a guard, not a path)
    return (uint32_t)idx;
}

__device__ __forceinline__ double pv_wave_sum_f64(double v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// One row per lane into the workgroup's table: `m` the lane holds a row, `cell` its table cell, `vok` its value cell counts
// (not null; for EXTREME not NaN), `val` the value (f64 bits, the i64, the order image, the row index).  Lanes holding the
// same cell as the first pending lane combine (the idiom of distinct.hip's dn_count), the rest add on their own.
template <int CLS>
__device__ __forceinline__ void pv_add(uint32_t *cnt, unsigned long long *state, uint32_t *nn, bool is_max, uint64_t identity,
                                       bool m, uint32_t cell, bool vok, uint64_t val) {
    uint64_t todo = __ballot(m);
    const uint32_t lane = threadIdx.x & 63;
    for (int round = 0; todo && round < PV_PEEL; round++) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint32_t c0 = __shfl(cell, leader, 64);
        const uint64_t same = __ballot(m && cell == c0) & todo;
        if (__popcll(same) < PV_PEEL_MIN) break;        // few lanes share a cell: they add on their own
        const bool mine = (same >> lane) & 1;
        const bool first = lane == (uint32_t)leader;
        if (first) atomicAdd(&cnt[c0], (uint32_t)__popcll(same));
        if (CLS != PV_CLS_ROWS) {
            const uint64_t counted = __ballot(mine && vok);
            if (CLS == PV_CLS_SUM_F64) {
                const double s = pv_wave_sum_f64(mine && vok ? __longlong_as_double((long long)val) : 0.0);
                if (first && counted) { atomicAdd(reinterpret_cast<double *>(&state[c0]), s); atomicAdd(&nn[c0], (uint32_t)__popcll(counted)); }
            } else if (CLS == PV_CLS_SUM_I64) {
                const uint64_t s = dn_wave_sum(mine && vok ? val : 0ull);
                if (first && counted) { atomicAdd(&state[c0], (unsigned long long)s); atomicAdd(&nn[c0], (uint32_t)__popcll(counted)); }
            } else if (is_max) {                        // (LAST: the largest row; `identity` 0)
                const uint64_t s = dn_wave_max(mine && vok ? val : identity);
                if (first && counted) atomicMax(&state[c0], (unsigned long long)s);
            } else {
                const uint64_t s = dn_wave_min(mine && vok ? val : identity);
                if (first && counted) atomicMin(&state[c0], (unsigned long long)s);
            }
        }
        todo &= ~same;
    }
    if ((todo >> lane) & 1) {
        atomicAdd(&cnt[cell], 1u);
        if (CLS != PV_CLS_ROWS && vok) {
            if (CLS == PV_CLS_SUM_F64) { atomicAdd(reinterpret_cast<double *>(&state[cell]), __longlong_as_double((long long)val)); atomicAdd(&nn[cell], 1u); }
            else if (CLS == PV_CLS_SUM_I64) { atomicAdd(&state[cell], (unsigned long long)val); atomicAdd(&nn[cell], 1u); }
            else if (is_max) atomicMax(&state[cell], (unsigned long long)val);
            else atomicMin(&state[cell], (unsigned long long)val);
        }
    }
}

// dynamic LDS: [state: cells x 8 bytes, unless ROWS] [cnt: cells x 4] [nn: cells x 4, the SUM classes].  The workspace table
// arrives initialised (rows 0, nn 0, state = a.init).
template <int CLS>
__global__ __launch_bounds__(PV_THREADS) void pv_stream_kernel(PvArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pv_smem[];
    const uint32_t R1 = a.n1 + 1, cells = R1 * (a.n2 + 1);
    constexpr bool HAS_STATE = CLS != PV_CLS_ROWS;
    constexpr bool HAS_NN = CLS == PV_CLS_SUM_F64 || CLS == PV_CLS_SUM_I64;
    unsigned long long *state = reinterpret_cast<unsigned long long *>(pv_smem);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(pv_smem + (HAS_STATE ? (size_t)cells * 8 : 0));
    uint32_t *nn = cnt + cells;
    for (uint32_t i = threadIdx.x; i < cells; i += PV_THREADS) {
        cnt[i] = 0;
        if (HAS_STATE) state[i] = a.init;
        if (HAS_NN) nn[i] = 0;
    }
    __syncthreads();
    const bool al1 = (reinterpret_cast<uintptr_t>(a.k1.data) & 15) == 0, al2 = (reinterpret_cast<uintptr_t>(a.k2.data) & 15) == 0;
    const bool alv = (reinterpret_cast<uintptr_t>(a.v.data) & 15) == 0;
    const bool is_max = a.is_max != 0;
    const int64_t n = a.k1.n;
    const int64_t tiles = (n + PV_TILE - 1) / PV_TILE;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t r0 = t * PV_TILE + 2 * (int64_t)threadIdx.x;
        uint64_t k1[PV_LOADS][2], k2[PV_LOADS][2], v[PV_LOADS][2];
        uint32_t in[PV_LOADS], nul1[PV_LOADS], nul2[PV_LOADS], nulv[PV_LOADS];
#pragma unroll
        for (int k = 0; k < PV_LOADS; k++) {                 // every load of the tile in flight before the first add
            const int64_t r = r0 + (int64_t)k * 2 * PV_THREADS;
            uint32_t in2;
            pv_load_key(a.dt1, a.k1, r, al1, k1[k], in[k]);
            pv_load_key(a.dt2, a.k2, r, al2, k2[k], in2);
            v[k][0] = v[k][1] = 0;
            if (HAS_STATE && CLS != PV_CLS_LAST) dn_load2<PANDRS_HIP_I64>(a.v, r, alv, v[k], in2);
            nul1[k] = a.k1.null && in[k] ? ((uint32_t)a.k1.null[r >> 3] >> (r & 7)) & 3 : 0;
            nul2[k] = a.k2.null && in[k] ? ((uint32_t)a.k2.null[r >> 3] >> (r & 7)) & 3 : 0;
            nulv[k] = HAS_STATE && CLS != PV_CLS_LAST && a.v.null && in[k] ? ((uint32_t)a.v.null[r >> 3] >> (r & 7)) & 3 : 0;
        }
#pragma unroll
        for (int k = 0; k < PV_LOADS; k++)                   // (a uniform loop: the ballots of pv_add see every lane)
#pragma unroll
            for (int j = 0; j < 2; j++) {
                bool m = (in[k] >> j) & 1;
                const uint32_t i1 = pv_slot(a.dt1, k1[k][j], (nul1[k] >> j) & 1, a.base1, a.n1, m);
                const uint32_t i2 = pv_slot(a.dt2, k2[k][j], (nul2[k] >> j) & 1, a.base2, a.n2, m);
                const uint32_t cell = m ? i2 * R1 + i1 : 0u;
                bool vok = !((nulv[k] >> j) & 1);
                uint64_t val = v[k][j];
                if (CLS == PV_CLS_EXTREME) {
                    if (a.v_i64) val = dn_image<PANDRS_HIP_I64>(val);
                    else { vok = vok && !dn_is_nan(val); val = dn_image<PANDRS_HIP_F64>(val); }
                }
                if (CLS == PV_CLS_LAST) val = (uint64_t)(r0 + (int64_t)k * 2 * PV_THREADS + j);
                pv_add<CLS>(cnt, state, nn, is_max || CLS == PV_CLS_LAST, a.init, m, cell, vok, val);
            }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < cells; i += PV_THREADS) {
        const uint32_t rows = cnt[i];
        if (!rows) continue;
        atomicAdd(&a.g_rows[i], (unsigned long long)rows);
        if (CLS == PV_CLS_SUM_F64) atomicAdd(reinterpret_cast<double *>(&a.g_state[i]), __longlong_as_double((long long)state[i]));
        if (CLS == PV_CLS_SUM_I64) atomicAdd(&a.g_state[i], state[i]);
        if (HAS_NN && nn[i]) atomicAdd(&a.g_nn[i], (unsigned long long)nn[i]);
        if (CLS == PV_CLS_EXTREME || CLS == PV_CLS_LAST) {
            if (is_max || CLS == PV_CLS_LAST) atomicMax(&a.g_state[i], state[i]); else atomicMin(&a.g_state[i], state[i]);
        }
    }
}

template <int DT>
__global__ __launch_bounds__(PV_THREADS) void pv_census_kernel(DnCol c, unsigned long long *census) {
    dn_census<DT, PV_THREADS, PV_LOADS>(c, census);
}

__global__ void pv_init_kernel(unsigned long long *g_rows, unsigned long long *g_state, unsigned long long *g_nn, uint32_t cells, uint64_t init) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cells) return;
    g_rows[i] = 0; g_state[i] = init; g_nn[i] = 0;
}

// the retained result: labels (8-byte cells as in distinct_fetch) and flags (0 number, 1 the missing label) of either dimension,
// the cells and the rows per cell, column-major
struct PvOut {
    uint64_t *ilab, *clab;
    uint8_t *iflag, *cflag;
    double *cells;
    int64_t *rows;
};

// The engine's finalisation (groupby.hip, finalize) of one cell from the direct table's states.
__device__ __forceinline__ double pv_finalize(int op, bool v_i64, uint64_t rows, uint64_t state, uint64_t nn, const DnCol &v) {
    switch (op) {
    case PANDRS_HIP_PIVOT_ROWS: case PANDRS_HIP_PIVOT_COUNT: return (double)rows;
    case PANDRS_HIP_PIVOT_SUM: return v_i64 ? (double)(int64_t)state : __longlong_as_double((long long)state);
    case PANDRS_HIP_PIVOT_MEAN:
        if (!nn) return 0.0;
        return (v_i64 ? (double)(int64_t)state : __longlong_as_double((long long)state)) / (double)nn;
    case PANDRS_HIP_PIVOT_MIN:
        if (v_i64) { const int64_t x = dec_i64(state); return x == INT64_MAX ? 0.0 : (double)x; }
        else { const double x = dec_f64(state); return x == __longlong_as_double(0x7FF0000000000000ll) ? 0.0 : x; }
    case PANDRS_HIP_PIVOT_MAX:
        if (v_i64) { const int64_t x = dec_i64(state); return x == INT64_MIN ? 0.0 : (double)x; }
        else { const double x = dec_f64(state); return x == __longlong_as_double((long long)0xFFF0000000000000ull) ? 0.0 : x; }
    default: {                                           // LAST: the value at the cell's largest row, null => 0.0
        const int64_t row = (int64_t)state;
        if (row < 0 || row >= v.n) return 0.0;           // (a row of the column: a guard, not a path)
        if (v.null && bit_at(v.null, row)) return 0.0;
        return v_i64 ? (double)static_cast<const int64_t *>(v.data)[row] : static_cast<const double *>(v.data)[row];
    }
    }
}

__device__ __forceinline__ int64_t pv_order_key(int dt, uint64_t cell, const DnRank &rk) {
    switch (dt) {
    case PANDRS_HIP_I64: return dn_order_key<PANDRS_HIP_I64>(cell, rk);
    case PANDRS_HIP_F64: return dn_order_key<PANDRS_HIP_F64>(cell, rk);
    case PANDRS_HIP_U32CODE: return dn_order_key<PANDRS_HIP_U32CODE>(cell, rk);
    default: return dn_order_key<PANDRS_HIP_BOOLBITS>(cell, rk);
    }
}

// the 8-byte cell of span slot s (I64 / code / bool: the number; F64: the integer as a double)
__device__ __forceinline__ uint64_t pv_slot_cell(int dt, uint64_t base, uint32_t s) {
    const uint64_t number = base + s;
    return dt == PANDRS_HIP_F64 ? (uint64_t)__double_as_longlong((double)(int64_t)number) : number;
}

// One workgroup: span rows and span columns without a row are dropped, the labels ordered (by rank for ranked codes), the dense
// R x C result written.  info[0] = R, [1] = C, [2] = cells with a row.  Slots 0 .. n1 are the index dimension (n1 = missing),
// slots n1 + 1 .. n1 + n2 + 1 the columns dimension.
__global__ __launch_bounds__(PV_FINISH_THREADS) void pv_finish_kernel(PvArgs a, int op, DnRank rk1, DnRank rk2, PvOut o, unsigned long long *info) {
    constexpr int SLOTS = PV_DIRECT_MAX_CELLS / 2 + 2;   // (n1 + 1) * (n2 + 1) <= PV_DIRECT_MAX_CELLS, either factor >= 2: the sum is at most this
    __shared__ int64_t ord[SLOTS];
    __shared__ uint32_t pos[SLOTS];
    __shared__ uint8_t occ[SLOTS];
    __shared__ uint32_t tot[3];
    const uint32_t R1 = a.n1 + 1, C1 = a.n2 + 1, cells = R1 * C1, slots = R1 + C1;
    for (uint32_t s = threadIdx.x; s < slots; s += PV_FINISH_THREADS) {
        occ[s] = 0;
        const bool col = s >= R1;
        const uint32_t k = col ? s - R1 : s;
        const bool missing = k == (col ? a.n2 : a.n1);
        ord[s] = missing ? INT64_MAX : (col ? pv_order_key(a.dt2, pv_slot_cell(a.dt2, a.base2, k), rk2) : pv_order_key(a.dt1, pv_slot_cell(a.dt1, a.base1, k), rk1));
    }
    if (threadIdx.x < 3) tot[threadIdx.x] = 0;
    __syncthreads();
    uint32_t present = 0;
    for (uint32_t i = threadIdx.x; i < cells; i += PV_FINISH_THREADS)
        if (a.g_rows[i]) { occ[i % R1] = 1; occ[R1 + i / R1] = 1; present++; }
    if (present) atomicAdd(&tot[2], present);
    __syncthreads();
    // a label's place: the occupied slots of its dimension that come before it (the missing label last)
    for (uint32_t s = threadIdx.x; s < slots; s += PV_FINISH_THREADS) {
        if (!occ[s]) continue;
        const bool col = s >= R1;
        const uint32_t lo = col ? R1 : 0, hi = col ? slots : R1, last = hi - 1;
        uint32_t before = 0;
        for (uint32_t q = lo; q < hi; q++) {
            if (!occ[q] || q == s) continue;
            const bool q_first = s == last ? true : (q == last ? false : (ord[q] < ord[s] || (ord[q] == ord[s] && q < s)));
            before += q_first ? 1u : 0u;
        }
        pos[s] = before;
        atomicAdd(&tot[col ? 1 : 0], 1u);
    }
    __syncthreads();
    const uint32_t R = tot[0];
    for (uint32_t s = threadIdx.x; s < slots; s += PV_FINISH_THREADS) {
        if (!occ[s]) continue;
        const bool col = s >= R1;
        const uint32_t k = col ? s - R1 : s;
        const bool missing = k == (col ? a.n2 : a.n1);
        const uint64_t cell = missing ? 0ull : (col ? pv_slot_cell(a.dt2, a.base2, k) : pv_slot_cell(a.dt1, a.base1, k));
        (col ? o.clab : o.ilab)[pos[s]] = cell;
        (col ? o.cflag : o.iflag)[pos[s]] = missing ? 1 : 0;
    }
    for (uint32_t i = threadIdx.x; i < cells; i += PV_FINISH_THREADS) {
        const uint32_t si = i % R1, sj = R1 + i / R1;
        if (!occ[si] || !occ[sj]) continue;
        const size_t at = (size_t)pos[sj] * R + pos[si];
        const uint64_t rows = a.g_rows[i];
        o.rows[at] = (int64_t)rows;
        o.cells[at] = rows ? pv_finalize(op, a.v_i64 != 0, rows, a.g_state[i], a.g_nn[i], a.v) : __longlong_as_double((long long)CANON_NAN);
    }
    if (threadIdx.x == 0) { info[0] = tot[0]; info[1] = tot[1]; info[2] = tot[2]; }
}

// ---- the general path ------------------------------------------------------------------------------------------------------------
// mask | (the cell is a NaN): a NaN key cell is the missing label like a null one, so the engine meets it under a null bit
__global__ void pv_nan_mask_kernel(const uint64_t *data, const uint8_t *null, int64_t n, uint8_t *out) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= (n + 7) / 8) return;
    uint32_t bits = null ? null[b] : 0u;
    for (int j = 0; j < 8; j++) {
        const int64_t r = b * 8 + j;
        if (r < n && dn_is_nan(data[r])) bits |= 1u << j;
    }
    out[b] = (uint8_t)bits;
}

// one column's groups -> unordered label entries: the cell, the class (0 number, 1 missing) and the order key as int64 sort keys
__global__ void pv_from_groups_kernel(int dt, const uint64_t *keys, const uint8_t *key_null, int64_t G, DnRank rk, uint64_t *cell,
                                      int64_t *cls, int64_t *ord) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const bool missing = key_null[g] || (dt == PANDRS_HIP_F64 && dn_is_nan(keys[g]));
    cell[g] = missing ? 0ull : keys[g];
    cls[g] = missing ? 1 : 0;
    ord[g] = missing ? 0 : pv_order_key(dt, keys[g], rk);
}

__global__ void pv_gather_labels_kernel(const uint64_t *cell, const int64_t *cls, const int64_t *ord, const int64_t *perm, int64_t G,
                                        uint64_t *out_cell, uint8_t *out_flag, int64_t *out_ord) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= G) return;
    const int64_t s = G > 1 ? perm[i] : 0;
    if (s < 0 || s >= G) return;                             // (a permutation of [0, G): a guard, not a path)
    out_cell[i] = cell[s]; out_flag[i] = (uint8_t)cls[s]; out_ord[i] = ord[s];
}

__global__ void pv_fill_kernel(double *cells, int64_t *rows, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    cells[i] = __longlong_as_double((long long)CANON_NAN);
    rows[i] = 0;
}

// the place of a group's key cell among the sorted labels: a binary search over the order keys of the numbers; the missing label
// is the last one.  -1: not listed (cannot happen: the lists come from the same column)
__device__ __forceinline__ int64_t pv_lookup(int dt, uint64_t cell, bool null, const DnRank &rk, const int64_t *ord, int64_t numbers, int64_t labels) {
    if (null || (dt == PANDRS_HIP_F64 && dn_is_nan(cell))) return labels > numbers ? numbers : -1;
    const int64_t key = pv_order_key(dt, cell, rk);
    int64_t lo = 0, hi = numbers;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (ord[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < numbers && ord[lo] == key ? lo : -1;
}

struct PvScatter {
    const uint64_t *keys;     // [2][cap]
    const uint8_t *key_null;  // [2][cap]
    const double *aggs;       // [n_aggs][cap]; the last one is COUNT
    int64_t G, cap;
    int32_t n_aggs, dt1, dt2;
    DnRank rk1, rk2;
    const int64_t *ord1, *ord2;
    int64_t num1, num2, R, C;
};
__global__ void pv_scatter_kernel(PvScatter s, double *cells, int64_t *rows, unsigned long long *lost) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= s.G) return;
    const int64_t i = pv_lookup(s.dt1, s.keys[g], s.key_null[g] != 0, s.rk1, s.ord1, s.num1, s.R);
    const int64_t j = pv_lookup(s.dt2, s.keys[s.cap + g], s.key_null[s.cap + g] != 0, s.rk2, s.ord2, s.num2, s.C);
    if (i < 0 || j < 0) { atomicAdd(lost, 1ull); return; }
    const size_t at = (size_t)j * s.R + i;
    rows[at] = (int64_t)s.aggs[(size_t)(s.n_aggs - 1) * s.cap + g];          // exact: a count below 2^32
    cells[at] = s.aggs[g];
}

struct PvLabels {
    uint64_t *cell = nullptr;
    uint8_t *flag = nullptr;
    int64_t *ord = nullptr;
    int64_t n = 0, numbers = 0;
};

// The label list of one key column on the general path: the engine lists the column's distinct cells, the radix sort orders them.
static int32_t pv_engine_labels(pandrs_hip_ctx *c, Arena &arena, const KeyDesc &key, int dt, const DnRank &rk, int64_t n_rows, PvLabels *out) {
    const pandrs_hip_agg_spec count{0, PANDRS_HIP_AGG_COUNT};
    Plan pl;
    const int32_t no_dtype = PANDRS_HIP_I64;                  // (COUNT reads no value column: the plan has no source)
    const uint8_t no_nulls = 0;
    ST_TRY(build_plan(&no_dtype, &no_nulls, 1, &count, 1, pl));
    RowSource rs;
    rs.n_rows = n_rows;
    rs.key = key;
    ST_TRY(run_engine(c, rs, pl, /*merge=*/false, /*partials=*/false, 1, dt, 1));
    const GroupbyResult &g = c->gb;
    if (!g.valid) return fail(PANDRS_HIP_ERR_COMPUTATION, "pivot: the engine left no result");
    const int64_t G = g.n_groups;
    out->n = G;
    if (G > PV_MAX_CELLS) return 0;                           // (too many labels for any result: the caller refuses)
    const size_t cap = (size_t)G + 1;
    ST_TRY(arena.ensure(5 * Arena::padded(cap * 8) + Arena::padded(cap), c->stream));
    uint64_t *cell = arena.take<uint64_t>(cap);
    int64_t *cls = arena.take<int64_t>(cap), *ord = arena.take<int64_t>(cap);
    out->cell = arena.take<uint64_t>(cap);
    out->ord = arena.take<int64_t>(cap);
    out->flag = arena.take<uint8_t>(cap);
    if (!cell || !cls || !ord || !out->cell || !out->ord || !out->flag) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (pivot)");
    if (!G) return 0;
    const unsigned blocks = (unsigned)((G + 255) / 256);
    {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_GATHER);
        hipLaunchKernelGGL(pv_from_groups_kernel, dim3(blocks), dim3(256), 0, c->stream, dt, g.keys, g.key_null, G, rk, cell, cls, ord);
        HIP_TRY(hipGetLastError());
    }
    int64_t *perm = nullptr;
    if (G > 1) {
        const KeyDesc keys[2] = {KeyDesc{cls, nullptr, nullptr, PANDRS_HIP_I64}, KeyDesc{ord, nullptr, nullptr, PANDRS_HIP_I64}};
        const int32_t asc[2] = {1, 1};
        ST_TRY(sort_order_device(c, keys, 2, asc, nullptr, 0, G, nullptr, 4096, &perm));
    }
    PhaseTimer pt(c, PANDRS_HIP_PHASE_GATHER);
    hipLaunchKernelGGL(pv_gather_labels_kernel, dim3(blocks), dim3(256), 0, c->stream, cell, cls, ord, perm, G, out->cell, out->flag, out->ord);
    HIP_TRY(hipGetLastError());
    return 0;
}

#define PV_CLS_DISPATCH(cls, CALL)                                                  \
    switch (cls) {                                                                  \
    case PV_CLS_ROWS: { constexpr int CLS = PV_CLS_ROWS; CALL; break; }             \
    case PV_CLS_SUM_F64: { constexpr int CLS = PV_CLS_SUM_F64; CALL; break; }       \
    case PV_CLS_SUM_I64: { constexpr int CLS = PV_CLS_SUM_I64; CALL; break; }       \
    case PV_CLS_EXTREME: { constexpr int CLS = PV_CLS_EXTREME; CALL; break; }       \
    default: { constexpr int CLS = PV_CLS_LAST; CALL; break; }                      \
    }

static size_t pv_result_bytes(size_t R, size_t C) {
    return 2 * Arena::padded(R * C * 8 + 8) + Arena::padded(R * 8 + 8) + Arena::padded(C * 8 + 8) + Arena::padded(R + 8) + Arena::padded(C + 8);
}
static bool pv_take_result(Arena &a, size_t R, size_t C, PvOut *o) {
    o->cells = a.take<double>(R * C + 1);
    o->rows = a.take<int64_t>(R * C + 1);
    o->ilab = a.take<uint64_t>(R + 1);
    o->clab = a.take<uint64_t>(C + 1);
    o->iflag = a.take<uint8_t>(R + 8);
    o->cflag = a.take<uint8_t>(C + 8);
    return o->cells && o->rows && o->ilab && o->clab && o->iflag && o->cflag;
}

static bool pv_key_dtype(int dt) { return dt == PANDRS_HIP_I64 || dt == PANDRS_HIP_F64 || dt == PANDRS_HIP_U32CODE || dt == PANDRS_HIP_BOOLBITS; }

int32_t pivot_entry(pandrs_hip_ctx *c, int32_t mem_space, const pandrs_hip_column *index_col, const uint32_t *index_rank, int64_t n_index_codes,
                    const pandrs_hip_column *columns_col, const uint32_t *columns_rank, int64_t n_columns_codes,
                    const pandrs_hip_column *values_col, int64_t n_rows, int32_t op, pandrs_hip_pivot_info *out_info) {
    if (!c || !index_col || !columns_col || !out_info || n_rows < 0 || n_index_codes < 0 || n_columns_codes < 0 ||
        (n_rows > 0 && (!index_col->data || !columns_col->data)))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "pivot: bad arguments");
    ST_TRY(check_mem_space("pivot", mem_space));
    if (op < PANDRS_HIP_PIVOT_ROWS || op > PANDRS_HIP_PIVOT_LAST)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "pivot: op %d (PANDRS_HIP_PIVOT_ROWS .. PANDRS_HIP_PIVOT_LAST)", op);
    if (op == PANDRS_HIP_PIVOT_ROWS && values_col)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "pivot: PANDRS_HIP_PIVOT_ROWS takes no values column");
    if (op != PANDRS_HIP_PIVOT_ROWS && !values_col)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "pivot: op %d needs a values column", op);
    const int dt1 = index_col->dtype, dt2 = columns_col->dtype;
    if (!pv_key_dtype(dt1) || !pv_key_dtype(dt2))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "pivot: the key columns have dtype %d and %d (I64, F64, U32CODE or BOOLBITS)", dt1, dt2);
    if (values_col && values_col->dtype != PANDRS_HIP_I64 && values_col->dtype != PANDRS_HIP_F64)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "pivot: the values column has dtype %d (I64 or F64)", values_col->dtype);
    if (values_col && n_rows > 0 && !values_col->data) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "pivot: the values column has no data");
    if ((index_rank && (dt1 != PANDRS_HIP_U32CODE || n_index_codes == 0)) || (columns_rank && (dt2 != PANDRS_HIP_U32CODE || n_columns_codes == 0)))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "pivot: a rank table needs a U32CODE column and n_codes > 0");
    if (n_rows >= (int64_t(1) << 32))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "pivot: %lld rows; one call takes fewer than 2^32", (long long)n_rows);
    std::lock_guard<std::mutex> lock(c->mu);
    *out_info = pandrs_hip_pivot_info{};
    PivotResult &res = c->pv;
    res = PivotResult{};
    c->gb.valid = false;                                     // whichever path answers: one contract
    HIP_TRY(hipSetDevice(c->device));
    timings_begin(c);                                        // (drops the retained distinct list and pivot result)
    if (n_rows == 0) {                                       // an empty result, and a record of its own like any other call
        ST_TRY(timings_end(c));
        res.valid = true;
        return 0;
    }
    const bool has_v = values_col != nullptr;
    const bool v_i64 = has_v && values_col->dtype == PANDRS_HIP_I64;

    ColView cv1{index_col->data, index_col->null_mask}, cv2{columns_col->data, columns_col->null_mask}, cvv{nullptr, nullptr};
    if (has_v) cvv = ColView{values_col->data, values_col->null_mask};
    const uint32_t *d_rank1 = index_rank, *d_rank2 = columns_rank;
    Stager stg{c, mem_space};
    const size_t rb1 = index_rank ? (size_t)n_index_codes * 4 : 0, rb2 = columns_rank ? (size_t)n_columns_codes * 4 : 0;
    if (const size_t need = stg.col_size(*index_col, n_rows) + stg.col_size(*columns_col, n_rows) + (has_v ? stg.col_size(*values_col, n_rows) : 0) +
                            stg.in_size(index_rank, rb1) + stg.in_size(columns_rank, rb2)) {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_STAGE_IN);
        ST_TRY(stg.reserve(need));
        cv1 = stg.col(*index_col, n_rows);
        cv2 = stg.col(*columns_col, n_rows);
        if (has_v) cvv = stg.col(*values_col, n_rows);
        d_rank1 = static_cast<const uint32_t *>(stg.in(index_rank, rb1));
        d_rank2 = static_cast<const uint32_t *>(stg.in(columns_rank, rb2));
        if (stg.status) return stg.status;
    }
    auto misaligned = [](int dt, const void *p) {
        return ((dt == PANDRS_HIP_I64 || dt == PANDRS_HIP_F64) && (reinterpret_cast<uintptr_t>(p) & 7)) || (dt == PANDRS_HIP_U32CODE && (reinterpret_cast<uintptr_t>(p) & 3));
    };
    if (misaligned(dt1, cv1.data) || misaligned(dt2, cv2.data) || (has_v && misaligned(PANDRS_HIP_I64, cvv.data)))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "pivot: I64 / F64 columns must be 8-byte aligned, codes 4-byte aligned");

    // ---- census of both key columns.  The workspace of this stage and of the direct table does not grow with n_rows.
    const size_t head_bytes = Arena::padded(2 * DN_CENSUS_WORDS * 8) + 3 * Arena::padded((size_t)PV_DIRECT_MAX_CELLS * 8) + Arena::padded(32);
    ST_TRY(c->work.ensure(head_bytes, c->stream));
    unsigned long long *d_census = c->work.take<unsigned long long>(2 * DN_CENSUS_WORDS);
    unsigned long long *g_rows = c->work.take<unsigned long long>(PV_DIRECT_MAX_CELLS);
    unsigned long long *g_state = c->work.take<unsigned long long>(PV_DIRECT_MAX_CELLS);
    unsigned long long *g_nn = c->work.take<unsigned long long>(PV_DIRECT_MAX_CELLS);
    unsigned long long *d_info = c->work.take<unsigned long long>(4);
    if (!d_census || !g_rows || !g_state || !g_nn || !d_info) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (pivot)");
    const DnCol dc1{cv1.data, cv1.mask, n_rows}, dc2{cv2.data, cv2.mask, n_rows}, dcv{cvv.data, cvv.mask, n_rows};
    const int64_t tiles = (n_rows + PV_TILE - 1) / PV_TILE;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)c->n_cu * PV_BLOCKS_PER_CU, tiles));
    uint64_t *pin = static_cast<uint64_t *>(c->pinned);
    uint64_t cs[2][DN_CENSUS_WORDS];
    {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_ESTIMATE);
        for (int k = 0; k < 2; k++) {
            pin[k * DN_CENSUS_WORDS + DN_MIN] = ~0ull;
            for (int i = 1; i < DN_CENSUS_WORDS; i++) pin[k * DN_CENSUS_WORDS + i] = 0;
        }
        HIP_TRY(hipMemcpyAsync(d_census, pin, 2 * DN_CENSUS_WORDS * 8, hipMemcpyHostToDevice, c->stream));
        DN_DISPATCH(dt1, hipLaunchKernelGGL(pv_census_kernel<DT>, dim3(grid), dim3(PV_THREADS), 0, c->stream, dc1, d_census));
        DN_DISPATCH(dt2, hipLaunchKernelGGL(pv_census_kernel<DT>, dim3(grid), dim3(PV_THREADS), 0, c->stream, dc2, d_census + DN_CENSUS_WORDS));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(pin, d_census, 2 * DN_CENSUS_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        std::memcpy(cs, pin, sizeof cs);
    }
    int64_t missing[2];
    for (int k = 0; k < 2; k++) {
        missing[k] = (int64_t)(cs[k][DN_NAN] + cs[k][DN_NULL]);
        if (missing[k] + (int64_t)cs[k][DN_VALID] != n_rows)
            return fail(PANDRS_HIP_ERR_COMPUTATION, "pivot: the census counted %lld of %lld rows", (long long)(missing[k] + (int64_t)cs[k][DN_VALID]), (long long)n_rows);
        const int64_t n_codes = k ? n_columns_codes : n_index_codes;
        if ((k ? dt2 : dt1) == PANDRS_HIP_U32CODE && n_codes > 0 && cs[k][DN_VALID] && cs[k][DN_MAX] >= (uint64_t)n_codes)
            return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "pivot: the %s column holds a string code >= n_codes (%lld)", k ? "columns" : "index", (long long)n_codes);
    }
    out_info->index_missing_rows = missing[0];
    out_info->column_missing_rows = missing[1];

    // ---- which path: either column's numbers as a span of slots, one more slot for the missing label
    uint64_t base1 = 0, base2 = 0, span1 = 0, span2 = 0;
    bool can_direct = dn_span(dt1, cs[0], &base1, &span1) && dn_span(dt2, cs[1], &base2, &span2) && span1 < (uint64_t)PV_DIRECT_MAX_CELLS &&
                      span2 < (uint64_t)PV_DIRECT_MAX_CELLS;
    can_direct = can_direct && (span1 + 2) * (span2 + 2) <= (uint64_t)PV_DIRECT_MAX_CELLS;
    const bool direct = can_direct && c->opt.pivot_path != 2;  // 1 and 0: direct wherever possible; 2: always the general path
    const DnRank rk1{d_rank1, (uint64_t)n_index_codes}, rk2{d_rank2, (uint64_t)n_columns_codes};
    const int64_t key_bytes = [&] {
        int64_t b = 0;
        for (int k = 0; k < 2; k++) {
            const int dt = k ? dt2 : dt1;
            b += n_rows * (int64_t)(dt == PANDRS_HIP_U32CODE ? 4 : (dt == PANDRS_HIP_BOOLBITS ? 0 : 8)) + ((k ? cv2.mask : cv1.mask) ? (n_rows + 7) / 8 : 0);
        }
        return b;
    }();
    const int64_t value_bytes = has_v && op != PANDRS_HIP_PIVOT_COUNT ? n_rows * 8 + (cvv.mask ? (n_rows + 7) / 8 : 0) : 0;

    PvOut o{};
    int64_t R = 0, C = 0, present = 0;
    if (direct) {
        PvArgs a{};
        a.k1 = dc1; a.k2 = dc2; a.v = dcv;
        a.dt1 = dt1; a.dt2 = dt2;
        a.v_i64 = v_i64 ? 1 : 0;
        a.is_max = op == PANDRS_HIP_PIVOT_MAX ? 1 : 0;
        a.base1 = base1; a.base2 = base2;
        a.n1 = (uint32_t)span1 + 1; a.n2 = (uint32_t)span2 + 1;
        a.g_rows = g_rows; a.g_state = g_state; a.g_nn = g_nn;
        int cls = PV_CLS_ROWS;
        size_t cell_bytes = 4;
        if (op == PANDRS_HIP_PIVOT_SUM || op == PANDRS_HIP_PIVOT_MEAN) { cls = v_i64 ? PV_CLS_SUM_I64 : PV_CLS_SUM_F64; cell_bytes = 16; }
        else if (op == PANDRS_HIP_PIVOT_MIN) { cls = PV_CLS_EXTREME; cell_bytes = 12; a.init = v_i64 ? ~0ull : 0xFFF0000000000000ull; }          // the image of I64_MAX / +inf
        else if (op == PANDRS_HIP_PIVOT_MAX) { cls = PV_CLS_EXTREME; cell_bytes = 12; a.init = v_i64 ? 0ull : 0x000FFFFFFFFFFFFFull; }           // the image of I64_MIN / -inf
        else if (op == PANDRS_HIP_PIVOT_LAST) { cls = PV_CLS_LAST; cell_bytes = 12; }
        const uint32_t cells = (a.n1 + 1) * (a.n2 + 1);
        ST_TRY(c->pv_arena.ensure(pv_result_bytes(a.n1 + 1, a.n2 + 1), c->stream));
        if (!pv_take_result(c->pv_arena, a.n1 + 1, a.n2 + 1, &o)) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (pivot)");
        {
            PhaseTimer pt(c, PANDRS_HIP_PHASE_AGGREGATE);
            hipLaunchKernelGGL(pv_init_kernel, dim3((cells + 255) / 256), dim3(256), 0, c->stream, g_rows, g_state, g_nn, cells, a.init);
            PV_CLS_DISPATCH(cls, hipLaunchKernelGGL(pv_stream_kernel<CLS>, dim3(grid), dim3(PV_THREADS), (size_t)cells * cell_bytes, c->stream, a));
            HIP_TRY(hipGetLastError());
        }
        {
            PhaseTimer pt(c, PANDRS_HIP_PHASE_GATHER);
            hipLaunchKernelGGL(pv_finish_kernel, dim3(1), dim3(PV_FINISH_THREADS), 0, c->stream, a, op, rk1, rk2, o, d_info);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(pin, d_info, 24, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        R = (int64_t)pin[0]; C = (int64_t)pin[1]; present = (int64_t)pin[2];
        if (R < 1 || C < 1 || R > (int64_t)a.n1 + 1 || C > (int64_t)a.n2 + 1 || present < 1 || present > R * C)
            return fail(PANDRS_HIP_ERR_COMPUTATION, "pivot: %lld x %lld labels, %lld cells from a %u x %u table", (long long)R, (long long)C, (long long)present, a.n1 + 1, a.n2 + 1);
    } else {
        c->jn.valid = false;                                 // the engine's result arena is the join result's
        // a NaN key cell goes under a null bit: the engine then meets ONE missing group per column
        const uint8_t *mask[2] = {cv1.mask, cv2.mask};
        {
            const size_t mb = (size_t)(n_rows + 7) / 8;
            const bool fix[2] = {dt1 == PANDRS_HIP_F64 && cs[0][DN_NAN] > 0, dt2 == PANDRS_HIP_F64 && cs[1][DN_NAN] > 0};
            if (fix[0] || fix[1]) {
                PhaseTimer pt(c, PANDRS_HIP_PHASE_OTHER);
                ST_TRY(c->pv_mask.ensure(2 * Arena::padded(mb), c->stream));
                for (int k = 0; k < 2; k++) {
                    if (!fix[k]) continue;
                    uint8_t *m = c->pv_mask.take<uint8_t>(mb);
                    if (!m) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (pivot)");
                    hipLaunchKernelGGL(pv_nan_mask_kernel, dim3((unsigned)((mb + 255) / 256)), dim3(256), 0, c->stream,
                                       static_cast<const uint64_t *>(k ? cv2.data : cv1.data), mask[k], n_rows, m);
                    mask[k] = m;
                }
                HIP_TRY(hipGetLastError());
            }
        }
        PvLabels lab[2];
        ST_TRY(pv_engine_labels(c, c->pv_lab0, KeyDesc{cv1.data, mask[0], nullptr, dt1}, dt1, rk1, n_rows, &lab[0]));
        ST_TRY(pv_engine_labels(c, c->pv_lab1, KeyDesc{cv2.data, mask[1], nullptr, dt2}, dt2, rk2, n_rows, &lab[1]));
        c->gb.valid = false;
        R = lab[0].n; C = lab[1].n;
        lab[0].numbers = R - (missing[0] ? 1 : 0);
        lab[1].numbers = C - (missing[1] ? 1 : 0);
        out_info->n_index_labels = R;
        out_info->n_column_labels = C;
        out_info->path = 2;
        if (R > PV_MAX_CELLS || C > PV_MAX_CELLS || R * C > PV_MAX_CELLS) {
            ST_TRY(timings_end(c));
            c->timings.n_partitions = 2;
            return fail(PANDRS_HIP_ERR_OPERATION_FAILED, "pivot: %lld x %lld labels are more than pivot_max_cells (%lld) cells", (long long)R, (long long)C, (long long)PV_MAX_CELLS);
        }
        // the engine over the two key columns: the op and the rows per group
        pandrs_hip_column keys[2] = {pandrs_hip_column{cv1.data, mask[0], dt1, 0}, pandrs_hip_column{cv2.data, mask[1], dt2, 0}};
        pandrs_hip_column val{cvv.data, cvv.mask, has_v ? values_col->dtype : PANDRS_HIP_I64, 0};
        static const int32_t engine_op[] = {PANDRS_HIP_AGG_COUNT, PANDRS_HIP_AGG_SUM, PANDRS_HIP_AGG_MEAN, PANDRS_HIP_AGG_MIN, PANDRS_HIP_AGG_MAX,
                                            PANDRS_HIP_AGG_COUNT, PANDRS_HIP_AGG_LAST};
        pandrs_hip_agg_spec aggs[2] = {{0, engine_op[op]}, {0, PANDRS_HIP_AGG_COUNT}};
        const bool counts_only = engine_op[op] == PANDRS_HIP_AGG_COUNT;
        const int n_aggs = counts_only ? 1 : 2, n_vals = 1;  // (COUNT alone reads no value column: the plan has no source)
        const int32_t vdt = val.dtype;
        const uint8_t vnull = val.null_mask != nullptr;
        Plan pl;
        ST_TRY(build_plan(&vdt, &vnull, n_vals, counts_only ? aggs + 1 : aggs, n_aggs, pl));
        ST_TRY(groupby_run(c, PANDRS_HIP_MEM_DEVICE, keys, 2, n_rows, &val, n_vals, counts_only ? aggs + 1 : aggs, n_aggs, false, pl));
        const GroupbyResult &g = c->gb;
        if (!g.valid) return fail(PANDRS_HIP_ERR_COMPUTATION, "pivot: the engine left no result");
        present = g.n_groups;
        ST_TRY(c->pv_arena.ensure(pv_result_bytes((size_t)R, (size_t)C) + Arena::padded(16), c->stream));
        unsigned long long *d_lost = c->pv_arena.take<unsigned long long>(2);
        if (!pv_take_result(c->pv_arena, (size_t)R, (size_t)C, &o) || !d_lost) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (pivot)");
        {
            PhaseTimer pt(c, PANDRS_HIP_PHASE_GATHER);
            HIP_TRY(hipMemsetAsync(d_lost, 0, 8, c->stream));
            HIP_TRY(hipMemcpyAsync(o.ilab, lab[0].cell, (size_t)R * 8, hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(o.iflag, lab[0].flag, (size_t)R, hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(o.clab, lab[1].cell, (size_t)C * 8, hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(o.cflag, lab[1].flag, (size_t)C, hipMemcpyDeviceToDevice, c->stream));
            const int64_t n_cells = R * C;
            hipLaunchKernelGGL(pv_fill_kernel, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, c->stream, o.cells, o.rows, n_cells);
            PvScatter s{g.keys, g.key_null, g.aggs, g.n_groups, g.cap, n_aggs, dt1, dt2, rk1, rk2, lab[0].ord, lab[1].ord, lab[0].numbers, lab[1].numbers, R, C};
            if (g.n_groups > 0)
                hipLaunchKernelGGL(pv_scatter_kernel, dim3((unsigned)((g.n_groups + 255) / 256)), dim3(256), 0, c->stream, s, o.cells, o.rows, d_lost);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(pin, d_lost, 8, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        c->gb.valid = false;
        if (pin[0]) return fail(PANDRS_HIP_ERR_COMPUTATION, "pivot: %llu groups found no label", (unsigned long long)pin[0]);
    }
    ST_TRY(timings_end(c));
    c->timings.n_partitions = direct ? 1 : 2;                // which path answered: 1 = direct table, 2 = general
    c->timings.algorithmic_bytes = (direct ? 2 : 1) * key_bytes + value_bytes + R * C * 16 + (R + C) * 9;
    out_info->n_index_labels = R;
    out_info->n_column_labels = C;
    out_info->n_cells_present = present;
    out_info->path = direct ? 1 : 2;
    res.R = R; res.C = C;
    res.ilab = o.ilab; res.clab = o.clab; res.iflag = o.iflag; res.cflag = o.cflag; res.cells = o.cells; res.rows = o.rows;
    res.valid = true;
    return 0;
}

int32_t pivot_fetch_entry(pandrs_hip_ctx *c, int32_t out_mem_space, uint64_t *out_index_labels, uint8_t *out_index_flags,
                          uint64_t *out_column_labels, uint8_t *out_column_flags, double *out_cells, int64_t *out_rows) {
    if (!c) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "pivot_fetch: no context");
    ST_TRY(check_mem_space("pivot_fetch", out_mem_space));
    std::lock_guard<std::mutex> lock(c->mu);
    const PivotResult &r = c->pv;
    if (!r.valid) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "no pivot result retained in this context");
    const size_t R = (size_t)r.R, C = (size_t)r.C;
    if (!R || !C) return 0;
    HIP_TRY(hipSetDevice(c->device));
    const hipMemcpyKind kind = out_mem_space == PANDRS_HIP_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (out_index_labels) HIP_TRY(hipMemcpyAsync(out_index_labels, r.ilab, R * 8, kind, c->stream));
    if (out_index_flags) HIP_TRY(hipMemcpyAsync(out_index_flags, r.iflag, R, kind, c->stream));
    if (out_column_labels) HIP_TRY(hipMemcpyAsync(out_column_labels, r.clab, C * 8, kind, c->stream));
    if (out_column_flags) HIP_TRY(hipMemcpyAsync(out_column_flags, r.cflag, C, kind, c->stream));
    if (out_cells) HIP_TRY(hipMemcpyAsync(out_cells, r.cells, R * C * 8, kind, c->stream));
    if (out_rows) HIP_TRY(hipMemcpyAsync(out_rows, r.rows, R * C * 8, kind, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace pandrs
