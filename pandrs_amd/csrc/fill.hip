// fill.hip — missing cells of one numeric column repaired in row order, behind PandasCompatExt::fillna / fillna_method /
// interpolate / ffill / bfill (reference src/dataframe/pandas_compat/functions.rs:789-918, :3626-3683), gfx950, wave64.
//
// A cell is missing when its null bit is set or, for F64, when it is NaN.  Rows in tiles of FILL_TILE; row p0 + r * 256 + tid,
// so every load and store is coalesced and one wave ballot IS the 64-row word.
// 1. Valid bits.  One stream over the column and its mask (the mask alone for I64): one bit per row, and per tile its first and
//    its last valid row.
// 2. Carry.  One small workgroup: the exclusive prefix "last valid row to the left" and the exclusive suffix "first valid row
//    to the right" over the tile summaries.  Every hand-off between workgroups is a kernel boundary, as in the sort and the
//    rank: no workgroup waits for another.  Row 0 can be a source here, so "no valid row" is 0 in a row + 1 encoding on the
//    left and FILL_NONE on the right (rows stay below 2^32 - 1).
// 3. Apply.  Per tile the words give each row its previous valid row (highest set bit at or below it, else the carry) and its
//    next one (lowest set bit at or above it, else the carry from the right).  A valid row stores its own cell, a missing row
//    gathers its neighbour's (Linear: both ends), and the ballot of "still missing" is the output mask word.
// Value needs neither 1 nor 2: one kernel.  An I64 column without a mask has nothing missing: a copy (Linear: a conversion).
#include "engine.hpp"

#include <algorithm>

namespace pandrs {

#pragma clang fp contract(off)      // Linear is the reference's expression, every operation rounded on its own

constexpr int FILL_THREADS = 256;                       // 4 waves
constexpr int FILL_RPT = 8;                             // rows per thread in a tile
constexpr int FILL_TILE = FILL_THREADS * FILL_RPT;      // 2048 rows: fill_tile_rows of pandrs_hip.h
constexpr int FILL_WORDS = FILL_TILE / 64;              // valid words per tile
constexpr int FILL_BLOCKS_PER_CU = 4;                   // fill_blocks_per_cu of pandrs_hip.h
constexpr int FILL_CARRY_THREADS = 1024;
constexpr uint32_t FILL_NONE = 0xFFFFFFFFu;
static_assert(FILL_WORDS <= 64, "one wave summarises a tile's words");

struct FillCol {
    const uint64_t *data;
    const uint8_t *mask;    // null bits or nullptr
    int64_t n;
};

struct FillOut {
    uint64_t *data;
    uint8_t *mask;          // ceil(n / 8) bytes or nullptr
    uint32_t *n_missing;    // += the rows still missing
};

struct FillTiles {
    uint64_t *valid;        // [tiles][FILL_WORDS]: bit b of word j of tile t = row t * FILL_TILE + j * 64 + b is valid
    uint32_t *first;        // [tiles] its first valid row, FILL_NONE when it has none
    uint32_t *last;         // [tiles] its last valid row + 1, 0 when it has none
    uint32_t *prev_in;      // [tiles] the last valid row + 1 in the tiles to the left, 0 when there is none
    uint32_t *next_in;      // [tiles] the first valid row in the tiles to the right, FILL_NONE when there is none
    int64_t tiles;
};

template <bool IS_I64>
__device__ __forceinline__ bool fill_valid(const FillCol &c, int64_t row) {
    if (c.mask && bit_at(c.mask, row)) return false;
    return IS_I64 || (c.data[row] & 0x7FFFFFFFFFFFFFFFull) <= 0x7FF0000000000000ull;
}

// the 64-row word `b` of "still missing" bits that starts at row `row0`, written bytewise: lanes 0 .. 7 hold one byte each, and no
// byte at or past ceil(n / 8) is touched (rows past n are never missing, so the last byte's high bits are 0)
__device__ __forceinline__ void fill_store_word(uint8_t *mask, int64_t row0, int64_t n, uint64_t b, uint32_t lane) {
    const int64_t byte = (row0 >> 3) + lane;
    if (lane < 8 && byte < ((n + 7) >> 3)) mask[byte] = (uint8_t)(b >> (lane * 8));
}

template <bool IS_I64>
__global__ __launch_bounds__(FILL_THREADS) void fill_valid_kernel(FillCol c, FillTiles ft) {
    __shared__ uint64_t w[FILL_WORDS];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int64_t t = blockIdx.x; t < ft.tiles; t += gridDim.x) {
        const int64_t p0 = t * FILL_TILE;
        __syncthreads();                                // the previous tile's words are consumed
#pragma unroll
        for (int r = 0; r < FILL_RPT; r++) {            // (a uniform loop: the ballots see every lane)
            const int64_t p = p0 + r * FILL_THREADS + tid;
            const bool ok = p < c.n && fill_valid<IS_I64>(c, p);
            const uint64_t b = __ballot(ok);
            if (lane == 0) w[r * (FILL_THREADS / 64) + wave] = b;           // word (r * 256 + tid) / 64, bit lane
        }
        __syncthreads();
        if (wave == 0) {
            const uint64_t x = lane < FILL_WORDS ? w[lane] : 0;
            if (lane < FILL_WORDS) ft.valid[(size_t)t * FILL_WORDS + lane] = x;
            uint32_t fi = x ? (uint32_t)(p0 + lane * 64 + __builtin_ctzll(x)) : FILL_NONE;
            uint32_t la = x ? (uint32_t)(p0 + lane * 64 + 63 - __builtin_clzll(x) + 1) : 0;
            for (int o = 32; o >= 1; o >>= 1) {
                fi = min(fi, (uint32_t)__shfl_down(fi, o, 64));
                la = max(la, (uint32_t)__shfl_down(la, o, 64));
            }
            if (lane == 0) { ft.first[t] = fi; ft.last[t] = la; }
        }
    }
}

// One workgroup: thread i owns a contiguous range of tiles; the ranges' maxima / minima are scanned in LDS.
__global__ __launch_bounds__(FILL_CARRY_THREADS) void fill_carry_kernel(FillTiles ft) {
    __shared__ uint32_t s_max[FILL_CARRY_THREADS], s_min[FILL_CARRY_THREADS];
    const int tid = threadIdx.x;
    const int64_t per = (ft.tiles + FILL_CARRY_THREADS - 1) / FILL_CARRY_THREADS;
    const int64_t beg = tid * per < ft.tiles ? tid * per : ft.tiles, end = beg + per < ft.tiles ? beg + per : ft.tiles;
    uint32_t mx = 0, mn = FILL_NONE;
    for (int64_t t = beg; t < end; t++) { mx = max(mx, ft.last[t]); mn = min(mn, ft.first[t]); }
    s_max[tid] = mx; s_min[tid] = mn;
    __syncthreads();
    for (int o = 1; o < FILL_CARRY_THREADS; o <<= 1) {  // inclusive: max over threads <= tid, min over threads >= tid
        const uint32_t b = tid >= o ? s_max[tid - o] : 0;
        const uint32_t d = tid + o < FILL_CARRY_THREADS ? s_min[tid + o] : FILL_NONE;
        __syncthreads();
        s_max[tid] = max(s_max[tid], b); s_min[tid] = min(s_min[tid], d);
        __syncthreads();
    }
    uint32_t prev = tid ? s_max[tid - 1] : 0;
    uint32_t next = tid + 1 < FILL_CARRY_THREADS ? s_min[tid + 1] : FILL_NONE;
    for (int64_t t = beg; t < end; t++) {
        ft.prev_in[t] = prev;
        prev = max(prev, ft.last[t]);
    }
    for (int64_t t = end - 1; t >= beg; t--) {
        ft.next_in[t] = next;
        next = min(next, ft.first[t]);
    }
}

// the cell a row of the output holds: Linear writes f64 whatever the column
template <int METHOD, bool IS_I64>
__device__ __forceinline__ uint64_t fill_own(uint64_t v) {
    return METHOD == PANDRS_HIP_FILL_LINEAR && IS_I64 ? (uint64_t)__double_as_longlong((double)(int64_t)v) : v;
}
template <bool IS_I64>
__device__ __forceinline__ double fill_f64(uint64_t v) {
    return IS_I64 ? (double)(int64_t)v : __longlong_as_double((long long)v);
}

// METHOD is FFILL, BFILL or LINEAR
template <int METHOD, bool IS_I64>
__global__ __launch_bounds__(FILL_THREADS) void fill_apply_kernel(FillCol c, FillTiles ft, FillOut o) {
    constexpr bool NEED_PREV = METHOD != PANDRS_HIP_FILL_BFILL, NEED_NEXT = METHOD != PANDRS_HIP_FILL_FFILL;
    constexpr bool OUT_I64 = IS_I64 && METHOD != PANDRS_HIP_FILL_LINEAR;
    __shared__ uint64_t w[FILL_WORDS];
    __shared__ uint32_t wprev[FILL_WORDS], wnext[FILL_WORDS];   // carried into each word of the tile
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    uint32_t missing = 0;
    for (int64_t t = blockIdx.x; t < ft.tiles; t += gridDim.x) {
        const int64_t p0 = t * FILL_TILE;
        __syncthreads();                                // the previous tile's words are consumed
        if (tid < FILL_WORDS) w[tid] = ft.valid[(size_t)t * FILL_WORDS + tid];
        __syncthreads();
        if (NEED_PREV && tid == 0) {
            uint32_t prev = ft.prev_in[t];
            for (int j = 0; j < FILL_WORDS; j++) {
                wprev[j] = prev;
                const uint64_t x = w[j];
                if (x) prev = (uint32_t)(p0 + j * 64 + 63 - __builtin_clzll(x) + 1);
            }
        }
        if (NEED_NEXT && tid == 64) {
            uint32_t next = ft.next_in[t];
            for (int j = FILL_WORDS - 1; j >= 0; j--) {
                wnext[j] = next;
                const uint64_t x = w[j];
                if (x) next = (uint32_t)(p0 + j * 64 + __builtin_ctzll(x));
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < FILL_RPT; r++) {            // (a uniform loop: the ballots see every lane)
            const uint32_t j = r * (FILL_THREADS / 64) + wave;
            const int64_t p = p0 + j * 64 + lane;
            const bool in = p < c.n;
            const uint64_t x = w[j];
            bool gone = false;                          // still missing
            uint64_t v = 0;
            if (in && ((x >> lane) & 1)) v = fill_own<METHOD, IS_I64>(c.data[p]);
            else if (in) {
                const uint64_t le = x & (~0ull >> (63 - lane));             // valid rows at or below this one, in its word
                const uint64_t ge = x & (~0ull << lane);                    // valid rows at or above it
                int64_t s = -1, e = -1;
                if (NEED_PREV) s = le ? p0 + j * 64 + 63 - __builtin_clzll(le) : (int64_t)wprev[j] - 1;
                if (NEED_NEXT) e = ge ? p0 + j * 64 + __builtin_ctzll(ge) : (wnext[j] == FILL_NONE ? -1 : (int64_t)wnext[j]);
                // (a carried row lies inside the column by construction; the bound is a guard, not a path)
                if (NEED_PREV && (uint64_t)s >= (uint64_t)c.n) s = -1;
                if (NEED_NEXT && (uint64_t)e >= (uint64_t)c.n) e = -1;
                if (METHOD == PANDRS_HIP_FILL_FFILL) { if (s >= 0) v = c.data[s]; else gone = true; }
                else if (METHOD == PANDRS_HIP_FILL_BFILL) { if (e >= 0) v = c.data[e]; else gone = true; }
                else if (s >= 0 && e >= 0) {
                    const double a = fill_f64<IS_I64>(c.data[s]), b = fill_f64<IS_I64>(c.data[e]);
                    v = (uint64_t)__double_as_longlong(a + ((b - a) * (double)(p - s)) / (double)(e - s));    // functions.rs:889-894
                } else gone = true;
                if (gone) v = OUT_I64 ? 0 : CANON_NAN;
            }
            if (in) o.data[p] = v;
            const uint64_t b = __ballot(gone);
            if (o.mask) fill_store_word(o.mask, p0 + j * 64, c.n, b, lane);
            if (lane == 0) missing += (uint32_t)__popcll(b);
        }
    }
    if (lane == 0 && missing) atomicAdd(o.n_missing, missing);
}

// Value, and the conversion of an I64 column without a mask under Linear: out = missing ? fill : own cell.  `stays` = the filled
// rows are still missing (an F64 fill with NaN): they are written as the canonical NaN.
template <bool IS_I64, bool TO_F64>
__global__ __launch_bounds__(FILL_THREADS) void fill_value_kernel(FillCol c, int64_t tiles, uint64_t fill, int stays, FillOut o) {
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    uint32_t missing = 0;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t p0 = t * FILL_TILE;
#pragma unroll
        for (int r = 0; r < FILL_RPT; r++) {            // (a uniform loop: the ballots see every lane)
            const uint32_t j = r * (FILL_THREADS / 64) + wave;
            const int64_t p = p0 + j * 64 + lane;
            const bool in = p < c.n;
            const bool miss = in && !fill_valid<IS_I64>(c, p);
            if (in) {
                const uint64_t v = c.data[p];
                o.data[p] = miss ? fill : TO_F64 ? (uint64_t)__double_as_longlong((double)(int64_t)v) : v;
            }
            const uint64_t b = __ballot(miss && stays);
            if (o.mask) fill_store_word(o.mask, p0 + j * 64, c.n, b, lane);
            if (lane == 0) missing += (uint32_t)__popcll(b);
        }
    }
    if (lane == 0 && missing) atomicAdd(o.n_missing, missing);
}

// bytes of c->work one call takes: the valid bits, four u32 per tile and the counter
static size_t fill_workspace(size_t tiles) {
    return Arena::padded(4) + Arena::padded(tiles * FILL_WORDS * 8) + 4 * Arena::padded(tiles * 4);
}

static bool fill_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && na && nb && x < y + nb && y < x + na;
}

template <int METHOD, bool IS_I64>
static void fill_launch_apply(pandrs_hip_ctx *c, int grid, const FillCol &fc, const FillTiles &ft, const FillOut &fo) {
    hipLaunchKernelGGL((fill_apply_kernel<METHOD, IS_I64>), dim3(grid), dim3(FILL_THREADS), 0, c->stream, fc, ft, fo);
}

int32_t fill_entry(pandrs_hip_ctx *c, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows, int32_t method, uint64_t fill_bits,
                   int32_t out_mem_space, void *out_data, uint8_t *out_null_mask, int64_t *out_n_missing) {
    if (!c || !col || n_rows < 0 || (n_rows > 0 && (!col->data || !out_data)))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "fill: bad arguments");
    ST_TRY(check_mem_space("fill", mem_space, out_mem_space));
    if (method < PANDRS_HIP_FILL_FFILL || method > PANDRS_HIP_FILL_VALUE)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "fill: method %d is not a pandrs_hip_fill_method", method);
    if (col->dtype != PANDRS_HIP_I64 && col->dtype != PANDRS_HIP_F64)
        return fail(PANDRS_HIP_ERR_TYPE_MISMATCH, "fill: the column has dtype %d, expected I64 or F64", col->dtype);
    if (n_rows >= (int64_t(1) << 32))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "fill: %lld rows; one call takes fewer than 2^32", (long long)n_rows);
    if (out_n_missing) *out_n_missing = 0;
    if (n_rows == 0) return 0;
    const bool is_i64 = col->dtype == PANDRS_HIP_I64, out_i64 = is_i64 && method != PANDRS_HIP_FILL_LINEAR;
    if (!out_null_mask && out_i64 && col->null_mask && method != PANDRS_HIP_FILL_VALUE)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "fill: an I64 result of a masked column needs out_null_mask (a row that stays missing is written as 0)");
    const size_t n = (size_t)n_rows, nbytes = (n + 7) / 8;
    if (mem_space == out_mem_space)                     // missing rows gather from their neighbours: not in place
        for (const void *o : {(const void *)out_data, (const void *)out_null_mask})
            if (fill_overlap(o, o == out_data ? n * 8 : nbytes, col->data, n * 8) || fill_overlap(o, o == out_data ? n * 8 : nbytes, col->null_mask, nbytes))
                return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "fill: an output overlaps the column; the call cannot run in place");
    std::lock_guard<std::mutex> lock(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    timings_begin(c);

    ColView cv{col->data, col->null_mask};
    void *d_out = out_data;
    uint8_t *d_omask = out_null_mask;
    Stager stg{c, mem_space, out_mem_space};
    const bool stage_mask = out_null_mask && out_mem_space == PANDRS_HIP_MEM_HOST;      // the call's second output: its own slot
    if (const size_t need = stg.col_size(*col, n_rows) + stg.out_size(out_data, n * 8) + (stage_mask ? Stager::slot(nbytes) : 0)) {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_STAGE_IN);
        ST_TRY(stg.reserve(need));
        cv = stg.col(*col, n_rows);
        d_out = stg.out(out_data, n * 8);
        if (stage_mask) d_omask = stg.scratch<uint8_t>(nbytes);
        if (stg.status) return stg.status;
    }
    if ((reinterpret_cast<uintptr_t>(cv.data) | reinterpret_cast<uintptr_t>(d_out)) & 7)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "fill: the column and out_data must be 8-byte aligned");

    // ---- the counter, the valid bits and the tile summaries in one arena, sized up front ----
    const int64_t tiles = (n_rows + FILL_TILE - 1) / FILL_TILE;
    const bool nothing_missing = is_i64 && !cv.mask;
    const bool one_kernel = method == PANDRS_HIP_FILL_VALUE || nothing_missing;
    ST_TRY(c->work.ensure(one_kernel ? Arena::padded(4) : fill_workspace((size_t)tiles), c->stream));
    uint32_t *d_missing = c->work.take<uint32_t>(1);
    FillTiles ft{};
    ft.tiles = tiles;
    if (!one_kernel) {
        ft.valid = c->work.take<uint64_t>((size_t)tiles * FILL_WORDS);
        ft.first = c->work.take<uint32_t>((size_t)tiles); ft.last = c->work.take<uint32_t>((size_t)tiles);
        ft.prev_in = c->work.take<uint32_t>((size_t)tiles); ft.next_in = c->work.take<uint32_t>((size_t)tiles);
    }
    if (!d_missing || (!one_kernel && (!ft.valid || !ft.first || !ft.last || !ft.prev_in || !ft.next_in)))
        return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (fill)");

    const FillCol fc{static_cast<const uint64_t *>(cv.data), cv.mask, n_rows};
    const FillOut fo{static_cast<uint64_t *>(d_out), d_omask, d_missing};
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)c->n_cu * FILL_BLOCKS_PER_CU, tiles));
    const int64_t mask_in = cv.mask ? (int64_t)nbytes : 0, mask_out = d_omask ? (int64_t)nbytes : 0;
    int64_t bytes = 0;
    {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_AGGREGATE);
        HIP_TRY(hipMemsetAsync(d_missing, 0, 4, c->stream));
        if (nothing_missing && method != PANDRS_HIP_FILL_LINEAR) {                  // a copy
            HIP_TRY(hipMemcpyAsync(d_out, cv.data, n * 8, hipMemcpyDeviceToDevice, c->stream));
            if (d_omask) HIP_TRY(hipMemsetAsync(d_omask, 0, nbytes, c->stream));
            bytes = (int64_t)n * 16 + mask_out;
        } else if (one_kernel) {
            const bool stays = !is_i64 && (fill_bits & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull;     // an F64 fill with NaN
            const uint64_t cell = stays ? CANON_NAN : fill_bits;
            if (method == PANDRS_HIP_FILL_LINEAR)
                hipLaunchKernelGGL((fill_value_kernel<true, true>), dim3(grid), dim3(FILL_THREADS), 0, c->stream, fc, tiles, cell, 0, fo);
            else if (is_i64)
                hipLaunchKernelGGL((fill_value_kernel<true, false>), dim3(grid), dim3(FILL_THREADS), 0, c->stream, fc, tiles, cell, 0, fo);
            else
                hipLaunchKernelGGL((fill_value_kernel<false, false>), dim3(grid), dim3(FILL_THREADS), 0, c->stream, fc, tiles, cell, stays ? 1 : 0, fo);
            bytes = (int64_t)n * 16 + mask_in + mask_out;
        } else {
            if (is_i64) hipLaunchKernelGGL(fill_valid_kernel<true>, dim3(grid), dim3(FILL_THREADS), 0, c->stream, fc, ft);
            else hipLaunchKernelGGL(fill_valid_kernel<false>, dim3(grid), dim3(FILL_THREADS), 0, c->stream, fc, ft);
            hipLaunchKernelGGL(fill_carry_kernel, dim3(1), dim3(FILL_CARRY_THREADS), 0, c->stream, ft);
            switch (method * 2 + (is_i64 ? 1 : 0)) {
            case PANDRS_HIP_FILL_FFILL * 2: fill_launch_apply<PANDRS_HIP_FILL_FFILL, false>(c, grid, fc, ft, fo); break;
            case PANDRS_HIP_FILL_FFILL * 2 + 1: fill_launch_apply<PANDRS_HIP_FILL_FFILL, true>(c, grid, fc, ft, fo); break;
            case PANDRS_HIP_FILL_BFILL * 2: fill_launch_apply<PANDRS_HIP_FILL_BFILL, false>(c, grid, fc, ft, fo); break;
            case PANDRS_HIP_FILL_BFILL * 2 + 1: fill_launch_apply<PANDRS_HIP_FILL_BFILL, true>(c, grid, fc, ft, fo); break;
            case PANDRS_HIP_FILL_LINEAR * 2: fill_launch_apply<PANDRS_HIP_FILL_LINEAR, false>(c, grid, fc, ft, fo); break;
            default: fill_launch_apply<PANDRS_HIP_FILL_LINEAR, true>(c, grid, fc, ft, fo); break;
            }
            // the valid pass streams the mask and, for F64, the column, and writes the bits; the carry reads and writes 16 bytes
            // per tile; the apply reads the bits and the column (a gathered cell is a neighbour's: the same lines) and writes
            bytes = (is_i64 ? 0 : (int64_t)n * 8) + mask_in + 2 * (int64_t)(tiles * FILL_WORDS * 8) + tiles * 32 + (int64_t)n * 16 + mask_out;
        }
        HIP_TRY(hipGetLastError());
    }
    c->timings.algorithmic_bytes = bytes;
    ST_TRY(stg.copy_back(n * 8));
    if (stage_mask) HIP_TRY(hipMemcpyAsync(out_null_mask, d_omask, nbytes, hipMemcpyDeviceToHost, c->stream));
    uint32_t missing = 0;
    HIP_TRY(hipMemcpyAsync(&missing, d_missing, 4, hipMemcpyDeviceToHost, c->stream));
    ST_TRY(timings_end(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (out_n_missing) *out_n_missing = (int64_t)missing;
    return 0;
}

}  // namespace pandrs
