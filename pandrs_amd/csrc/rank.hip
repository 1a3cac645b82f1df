// rank.hip — the ascending 1-based rank of every row of one numeric column, behind PandasCompatExt::rank (reference
// src/dataframe/pandas_compat/functions.rs:193-236, RankMethod at pandas_compat/types.rs:48-59), gfx950, wave64.
//
// 1. Order.  The stable radix sort of sort.hip (sort_order_device) leaves the permutation perm[p] = row at sorted position p
//    on the device: numbers ascending, then NaN, then nulls.  A count of the rankable (non-NaN, non-null) cells gives m:
//    positions [0, m) hold the numbers.
// 2. Run starts.  Over sorted positions in tiles of RANK_TILE: position p < m starts a tie run iff p == 0 or the cell at
//    perm[p] differs from the cell at perm[p - 1] (the cells themselves: I64 as integers, F64 bits with -0.0 -> 0.0).  One
//    bit per position (a wave ballot IS the 64-position word), and per tile the number of starts and its first and last one.
// 3. Carry.  Two levels: one small workgroup scans the tile summaries (exclusive sum of the counts, exclusive prefix maximum of
//    the last starts, exclusive suffix minimum of the first starts, m where no run follows).  Every hand-off between
//    workgroups is a kernel boundary, as in the sort: no workgroup waits for another.
// 4. Apply and scatter.  Per tile the flag words give each position its run's start (highest set bit at or below it, else the
//    carry), the next run's start (lowest set bit above it, else the carry from the right) and the starts up to it; the
//    rank is built from those integers and written to out[perm[p]], NaN for p >= m.  First needs neither 2 nor 3.
#include "engine.hpp"

#include <algorithm>

namespace pandrs {

constexpr int RANK_THREADS = 256;                       // 4 waves
constexpr int RANK_RPT = 8;                             // positions per thread in a tile
constexpr int RANK_TILE = RANK_THREADS * RANK_RPT;      // 2048 positions: rank_tile_rows of pandrs_hip.h
constexpr int RANK_WORDS = RANK_TILE / 64;              // flag words per tile
constexpr int RANK_BLOCKS_PER_CU = 4;                   // rank_blocks_per_cu of pandrs_hip.h
constexpr int RANK_CARRY_THREADS = 1024;
constexpr uint32_t RANK_NONE = 0xFFFFFFFFu;
static_assert(RANK_WORDS <= 64, "one wave summarises a tile's flag words");

struct RankCol {
    const uint64_t *data;
    const uint8_t *mask;    // null bits or nullptr
    int64_t n;
    int is_i64;
};

__device__ __forceinline__ bool rank_rankable(const RankCol &c, int64_t row) {
    if (c.mask && bit_at(c.mask, row)) return false;
    return c.is_i64 || (c.data[row] & 0x7FFFFFFFFFFFFFFFull) <= 0x7FF0000000000000ull;
}

// the cell as ties compare it: the reference's `==` on two numbers
__device__ __forceinline__ uint64_t rank_cell(const RankCol &c, int64_t row) {
    const uint64_t b = c.data[row];
    return (!c.is_i64 && b == 0x8000000000000000ull) ? 0 : b;   // -0.0 == 0.0
}

// *m += the rankable cells
__global__ void rank_count_kernel(RankCol c, uint32_t *m) {
    uint32_t k = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < c.n; i += (int64_t)gridDim.x * blockDim.x)
        k += rank_rankable(c, i) ? 1u : 0u;
    for (int o = 32; o >= 1; o >>= 1) k += __shfl_down(k, o, 64);
    if ((threadIdx.x & 63) == 0 && k) atomicAdd(m, k);
}

struct RankTiles {
    uint64_t *flags;        // [tiles][RANK_WORDS]: bit b of word j of tile t = position t * RANK_TILE + j * 64 + b starts a run
    uint32_t *count;        // [tiles] starts in the tile
    uint32_t *first, *last; // [tiles] its first / last start (positions); RANK_NONE / 0 when it has none
    uint32_t *dense_in;     // [tiles] starts in the tiles to the left
    uint32_t *start_in;     // [tiles] the last start in the tiles to the left (the open run)
    uint32_t *next_in;      // [tiles] the first start in the tiles to the right, m when there is none
    int64_t tiles;
};

__global__ __launch_bounds__(RANK_THREADS) void rank_starts_kernel(RankCol c, const int64_t *perm, const uint32_t *m_ptr, RankTiles rt) {
    __shared__ uint64_t cell[RANK_TILE + 1];            // cell[0] = the cell in front of the tile
    __shared__ uint64_t w[RANK_WORDS];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t m = (int64_t)*m_ptr;
    for (int64_t t = blockIdx.x; t < rt.tiles; t += gridDim.x) {
        const int64_t p0 = t * RANK_TILE;
        __syncthreads();                                // the previous tile's cells and words are consumed
#pragma unroll
        for (int r = 0; r < RANK_RPT; r++) {
            const uint32_t li = r * RANK_THREADS + tid;
            const int64_t p = p0 + li;
            uint64_t v = 0;
            if (p < m) {
                const int64_t row = perm[p];
                if ((uint64_t)row < (uint64_t)c.n) v = rank_cell(c, row);   // (a permutation holds rows only; a guard, not a path)
            }
            cell[li + 1] = v;
        }
        if (tid == 0) {
            uint64_t v = 0;
            if (p0 > 0 && p0 < m) {
                const int64_t row = perm[p0 - 1];
                if ((uint64_t)row < (uint64_t)c.n) v = rank_cell(c, row);
            }
            cell[0] = v;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < RANK_RPT; r++) {            // (a uniform loop: the ballots see every lane)
            const uint32_t li = r * RANK_THREADS + tid;
            const int64_t p = p0 + li;
            const bool st = p < m && (p == 0 || cell[li + 1] != cell[li]);
            const uint64_t b = __ballot(st);
            if (lane == 0) w[r * (RANK_THREADS / 64) + wave] = b;           // word li / 64, bit lane
        }
        __syncthreads();
        if (wave == 0) {
            const uint64_t x = lane < RANK_WORDS ? w[lane] : 0;
            if (lane < RANK_WORDS) rt.flags[(size_t)t * RANK_WORDS + lane] = x;
            uint32_t cnt = (uint32_t)__popcll(x);
            uint32_t fi = x ? (uint32_t)(p0 + lane * 64 + __builtin_ctzll(x)) : RANK_NONE;
            uint32_t la = x ? (uint32_t)(p0 + lane * 64 + 63 - __builtin_clzll(x)) : 0;
            for (int o = 32; o >= 1; o >>= 1) {
                cnt += __shfl_down(cnt, o, 64);
                fi = min(fi, (uint32_t)__shfl_down(fi, o, 64));
                la = max(la, (uint32_t)__shfl_down(la, o, 64));
            }
            if (lane == 0) { rt.count[t] = cnt; rt.first[t] = fi; rt.last[t] = la; }
        }
    }
}

// One workgroup: thread i owns a contiguous range of tiles; the ranges' sums / maxima / minima are scanned in LDS.
__global__ __launch_bounds__(RANK_CARRY_THREADS) void rank_carry_kernel(RankTiles rt, const uint32_t *m_ptr) {
    __shared__ uint32_t s_sum[RANK_CARRY_THREADS], s_max[RANK_CARRY_THREADS], s_min[RANK_CARRY_THREADS];
    const int tid = threadIdx.x;
    const int64_t per = (rt.tiles + RANK_CARRY_THREADS - 1) / RANK_CARRY_THREADS;
    const int64_t beg = tid * per < rt.tiles ? tid * per : rt.tiles, end = beg + per < rt.tiles ? beg + per : rt.tiles;
    uint32_t sum = 0, mx = 0, mn = RANK_NONE;
    for (int64_t t = beg; t < end; t++) { sum += rt.count[t]; mx = max(mx, rt.last[t]); mn = min(mn, rt.first[t]); }
    s_sum[tid] = sum; s_max[tid] = mx; s_min[tid] = mn;
    __syncthreads();
    for (int o = 1; o < RANK_CARRY_THREADS; o <<= 1) {  // inclusive: sum and max over threads <= tid, min over threads >= tid
        const uint32_t a = tid >= o ? s_sum[tid - o] : 0, b = tid >= o ? s_max[tid - o] : 0;
        const uint32_t d = tid + o < RANK_CARRY_THREADS ? s_min[tid + o] : RANK_NONE;
        __syncthreads();
        s_sum[tid] += a; s_max[tid] = max(s_max[tid], b); s_min[tid] = min(s_min[tid], d);
        __syncthreads();
    }
    uint32_t dense = tid ? s_sum[tid - 1] : 0, start = tid ? s_max[tid - 1] : 0;
    uint32_t next = tid + 1 < RANK_CARRY_THREADS ? s_min[tid + 1] : RANK_NONE;
    next = min(next, *m_ptr);                            // no run to the right: the numbers end at m
    for (int64_t t = beg; t < end; t++) {
        rt.dense_in[t] = dense; rt.start_in[t] = start;
        dense += rt.count[t]; start = max(start, rt.last[t]);
    }
    for (int64_t t = end - 1; t >= beg; t--) {
        rt.next_in[t] = next;
        next = min(next, rt.first[t]);
    }
}

// out[perm[p]] = the rank of sorted position p; METHOD is a pandrs_hip_rank_method
template <int METHOD>
__global__ __launch_bounds__(RANK_THREADS) void rank_apply_kernel(const int64_t *perm, int64_t n, const uint32_t *m_ptr, RankTiles rt, double *out) {
    constexpr bool NEED_START = METHOD == PANDRS_HIP_RANK_AVERAGE || METHOD == PANDRS_HIP_RANK_MIN;
    constexpr bool NEED_END = METHOD == PANDRS_HIP_RANK_AVERAGE || METHOD == PANDRS_HIP_RANK_MAX;
    constexpr bool NEED_DENSE = METHOD == PANDRS_HIP_RANK_DENSE;
    __shared__ uint64_t w[RANK_WORDS];
    __shared__ uint32_t wstart[RANK_WORDS], wnext[RANK_WORDS], wdense[RANK_WORDS];   // carried into each word of the tile
    const uint32_t tid = threadIdx.x;
    const int64_t m = (int64_t)*m_ptr;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    for (int64_t t = blockIdx.x; t < rt.tiles; t += gridDim.x) {
        const int64_t p0 = t * RANK_TILE;
        if (METHOD != PANDRS_HIP_RANK_FIRST) {
            __syncthreads();                            // the previous tile's words are consumed
            if (tid < RANK_WORDS) w[tid] = rt.flags[(size_t)t * RANK_WORDS + tid];
            __syncthreads();
            if (tid == 0) {
                if (NEED_START || NEED_DENSE) {
                    uint32_t start = rt.start_in[t], dense = rt.dense_in[t];
                    for (int j = 0; j < RANK_WORDS; j++) {
                        wstart[j] = start; wdense[j] = dense;
                        const uint64_t x = w[j];
                        if (x) { start = (uint32_t)(p0 + j * 64 + 63 - __builtin_clzll(x)); dense += (uint32_t)__popcll(x); }
                    }
                }
                if (NEED_END) {
                    uint32_t next = rt.next_in[t];
                    for (int j = RANK_WORDS - 1; j >= 0; j--) {
                        wnext[j] = next;
                        const uint64_t x = w[j];
                        if (x) next = (uint32_t)(p0 + j * 64 + __builtin_ctzll(x));
                    }
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < RANK_RPT; r++) {
            const uint32_t li = r * RANK_THREADS + tid;
            const int64_t p = p0 + li;
            if (p >= n) continue;
            const int64_t row = perm[p];
            if ((uint64_t)row >= (uint64_t)n) continue;  // (a permutation holds rows only; a guard, not a path)
            double v;
            if (p >= m) v = nan;
            else if (METHOD == PANDRS_HIP_RANK_FIRST) v = (double)(p + 1);
            else {
                const uint32_t j = li >> 6, b = li & 63;
                const uint64_t x = w[j];
                const uint64_t le = x & (~0ull >> (63 - b));                 // starts at or below this position, in its word
                const uint64_t gt = b == 63 ? 0 : x & (~0ull << (b + 1));    // starts above it
                uint64_t s = 0, e = 0;
                if (NEED_START) s = le ? (uint64_t)(p0 + j * 64 + 63 - __builtin_clzll(le)) : wstart[j];
                if (NEED_END) e = gt ? (uint64_t)(p0 + j * 64 + __builtin_ctzll(gt)) : wnext[j];
                if (METHOD == PANDRS_HIP_RANK_AVERAGE) v = (double)(s + e + 1) * 0.5;   // integers below 2^33: exact
                else if (METHOD == PANDRS_HIP_RANK_MIN) v = (double)(s + 1);
                else if (METHOD == PANDRS_HIP_RANK_MAX) v = (double)e;
                else v = (double)((uint64_t)wdense[j] + (uint64_t)__popcll(le));
            }
            out[row] = v;
        }
    }
}

// bytes of c->work the rank phase takes on top of the sort's and the permutation (sort_order_device's extra_work)
static size_t rank_phase_workspace(size_t tiles) {
    return Arena::padded(4) + Arena::padded(tiles * RANK_WORDS * 8) + 6 * Arena::padded(tiles * 4);
}

int32_t rank_entry(pandrs_hip_ctx *c, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows, int32_t method,
                   int32_t out_mem_space, double *out) {
    if (!c || !col || n_rows < 0 || (n_rows > 0 && (!col->data || !out)))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "rank: bad arguments");
    ST_TRY(check_mem_space("rank", mem_space, out_mem_space));
    if (method < PANDRS_HIP_RANK_AVERAGE || method > PANDRS_HIP_RANK_DENSE)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "rank: method %d is not a pandrs_hip_rank_method", method);
    if (col->dtype != PANDRS_HIP_I64 && col->dtype != PANDRS_HIP_F64)
        return fail(PANDRS_HIP_ERR_TYPE_MISMATCH, "rank: the column has dtype %d, expected I64 or F64", col->dtype);
    if (n_rows >= (int64_t(1) << 32))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "rank: %lld rows; one call takes fewer than 2^32", (long long)n_rows);
    if (n_rows == 0) return 0;
    std::lock_guard<std::mutex> lock(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    timings_begin(c);
    const size_t n = (size_t)n_rows;

    ColView cv{col->data, col->null_mask};
    double *d_out = out;
    Stager stg{c, mem_space, out_mem_space};
    if (const size_t need = stg.col_size(*col, n_rows) + stg.out_size(out, n * 8)) {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_STAGE_IN);
        ST_TRY(stg.reserve(need));
        cv = stg.col(*col, n_rows);
        d_out = stg.out(out, n * 8);
        if (stg.status) return stg.status;
    }
    if ((reinterpret_cast<uintptr_t>(cv.data) | reinterpret_cast<uintptr_t>(d_out)) & 7)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "rank: the column and out must be 8-byte aligned");

    // ---- the order: the sort's workspace, the permutation and the rank phase's buffers in one arena, sized up front ----
    const int64_t tiles = (n_rows + RANK_TILE - 1) / RANK_TILE;
    const KeyDesc key{cv.data, cv.mask, nullptr, col->dtype};
    int64_t *perm = nullptr;
    ST_TRY(sort_order_device(c, &key, 1, nullptr, nullptr, 0, n_rows, nullptr, rank_phase_workspace((size_t)tiles), &perm));
    const int64_t sort_bytes = c->timings.algorithmic_bytes;
    uint32_t *d_m = c->work.take<uint32_t>(1);
    RankTiles rt{};
    rt.tiles = tiles;
    rt.flags = c->work.take<uint64_t>((size_t)tiles * RANK_WORDS);
    rt.count = c->work.take<uint32_t>((size_t)tiles); rt.first = c->work.take<uint32_t>((size_t)tiles); rt.last = c->work.take<uint32_t>((size_t)tiles);
    rt.dense_in = c->work.take<uint32_t>((size_t)tiles); rt.start_in = c->work.take<uint32_t>((size_t)tiles); rt.next_in = c->work.take<uint32_t>((size_t)tiles);
    if (!perm || !d_m || !rt.flags || !rt.count || !rt.first || !rt.last || !rt.dense_in || !rt.start_in || !rt.next_in)
        return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (rank)");

    const RankCol rc{static_cast<const uint64_t *>(cv.data), cv.mask, n_rows, col->dtype == PANDRS_HIP_I64 ? 1 : 0};
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)c->n_cu * RANK_BLOCKS_PER_CU, tiles));
    {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_AGGREGATE);
        HIP_TRY(hipMemsetAsync(d_m, 0, 4, c->stream));
        const int blocks_rd = (int)std::min<int64_t>(2048, (n_rows + 255) / 256);
        hipLaunchKernelGGL(rank_count_kernel, dim3(blocks_rd), dim3(256), 0, c->stream, rc, d_m);
        if (method != PANDRS_HIP_RANK_FIRST) {
            hipLaunchKernelGGL(rank_starts_kernel, dim3(grid), dim3(RANK_THREADS), 0, c->stream, rc, perm, d_m, rt);
            hipLaunchKernelGGL(rank_carry_kernel, dim3(1), dim3(RANK_CARRY_THREADS), 0, c->stream, rt, d_m);
        }
        switch (method) {
        case PANDRS_HIP_RANK_AVERAGE: hipLaunchKernelGGL(rank_apply_kernel<PANDRS_HIP_RANK_AVERAGE>, dim3(grid), dim3(RANK_THREADS), 0, c->stream, perm, n_rows, d_m, rt, d_out); break;
        case PANDRS_HIP_RANK_MIN: hipLaunchKernelGGL(rank_apply_kernel<PANDRS_HIP_RANK_MIN>, dim3(grid), dim3(RANK_THREADS), 0, c->stream, perm, n_rows, d_m, rt, d_out); break;
        case PANDRS_HIP_RANK_MAX: hipLaunchKernelGGL(rank_apply_kernel<PANDRS_HIP_RANK_MAX>, dim3(grid), dim3(RANK_THREADS), 0, c->stream, perm, n_rows, d_m, rt, d_out); break;
        case PANDRS_HIP_RANK_FIRST: hipLaunchKernelGGL(rank_apply_kernel<PANDRS_HIP_RANK_FIRST>, dim3(grid), dim3(RANK_THREADS), 0, c->stream, perm, n_rows, d_m, rt, d_out); break;
        default: hipLaunchKernelGGL(rank_apply_kernel<PANDRS_HIP_RANK_DENSE>, dim3(grid), dim3(RANK_THREADS), 0, c->stream, perm, n_rows, d_m, rt, d_out); break;
        }
        HIP_TRY(hipGetLastError());
    }
    // the count streams the column; the starts read the permutation and gather the cells; the apply reads it again and scatters
    c->timings.algorithmic_bytes = sort_bytes + (int64_t)n * (8 + (method != PANDRS_HIP_RANK_FIRST ? 16 : 0) + 16);
    ST_TRY(stg.copy_back(n * 8));
    ST_TRY(timings_end(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace pandrs
