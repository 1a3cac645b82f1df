// bin.hip — bin codes and per-bin counts of one numeric column, behind PandasCompatExt::cut / qcut (reference
// src/dataframe/pandas_compat/functions.rs:2339-2368, :2370-2420), gfx950, wave64.  The edge list itself comes from
// describe.hip (pandrs_hip_bin_edges); this file answers "which bin" for every row.
//
// The reference walks the bins and takes the FIRST i with v >= e[i] && v < e[i + 1].  With a non-decreasing edge list that is
// i = (number of edges <= v) - 1 whenever that lies in [0, n_bins): e[i] <= v < e[i + 1] names i uniquely, and a bin with
// e[i] == e[i + 1] is empty either way.  A cell is read in f64 (I64 `as f64`, per row); a NaN cell or a cell under a null
// bit is PANDRS_HIP_BIN_NAN and the cell under the bit is not looked at.
// One stream over the column in tiles of BIN_TILE rows, 16-byte loads (two rows per thread and load), codes stored as
// coalesced int32 pairs.  Every workgroup copies the edges into LDS once.
// 1. search: a branch-free upper bound, ceil(log2(n_bins + 1)) steps, the same count for every lane.
// 2. guess: when the host finds the edges evenly spaced, (int)((v - e[0]) / w) is clamped and corrected against the real
//    edges in LDS, at most BIN_FIX steps; a lane that is still wrong after them takes the search.  What a lane ends with
//    satisfies e[i] <= v < e[i + 1], so both paths give the same code for every row.
// Counts: a uint32 histogram of n_bins + 2 cells per workgroup in LDS (the bins, NONE, NAN); lanes of a wave holding the
// same code add once (the ballot peel of describe.hip's ds_count, given up as soon as a round folds fewer than BIN_PEEL_MIN
// lanes: rows spread over many bins gain nothing from it), the rest by plain LDS atomics; the non-zero cells are
// added to 64-bit workspace counters when the workgroup ends.  Integers: exact, whatever the order.  No workgroup waits
// for another.
#include "engine.hpp"

#include <algorithm>
#include <cmath>

namespace pandrs {

#pragma clang fp contract(off)

constexpr int BIN_THREADS = 256;
constexpr int BIN_LOADS = 4;                             // 16-byte loads in flight per thread
constexpr int BIN_TILE = BIN_THREADS * BIN_LOADS * 2;    // rows per workgroup iteration (2048; pandrs_hip.h: bin_tile_rows)
constexpr int BIN_BLOCKS_PER_CU = 4;                     // pandrs_hip.h: bin_blocks_per_cu
constexpr int BIN_MAX_BINS = PANDRS_HIP_BIN_MAX_BINS;    // pandrs_hip.h: bin_max_bins = 4096; (BIN_MAX_BINS + 1) x 8 bytes of edges in LDS
constexpr int BIN_PEEL = 4;                              // codes a wave folds by ballot before plain atomics
constexpr int BIN_PEEL_MIN = 4;                          // ... as long as a round folds at least this many lanes
constexpr int BIN_FIX = 2;                               // correction steps of the guess before it takes the search
constexpr int BIN_GUESS_MIN_BINS = 128;                  // "bin_path" 0: the guess from this many evenly spaced bins on (measured:
                                                         // the search wins at 64 bins and loses at 256, experiments/bin_bench.py)

struct BinCol {
    const uint64_t *data;     // 8-byte aligned
    const uint8_t *null;      // LSB-first, 1 = null, any byte offset
    int64_t n;
};

struct BinEdges {
    const double *edges;      // n_bins + 1, device
    int32_t n_bins;
    double e0, inv_w;         // the guess: (v - e0) * inv_w
};

__device__ __forceinline__ bool bin_is_nan(double v) {
    return ((uint64_t)__double_as_longlong(v) & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull;
}

// the number of edges e[0 .. n) that are <= v; the steps depend on n alone
__device__ __forceinline__ int bin_upper_bound(const double *e, int n, double v) {
    int base = 0, len = n;
    while (len > 1) {                                    // the answer lies in [base, base + len]
        const int half = len >> 1;
        base += e[base + half - 1] <= v ? half : 0;
        len -= half;
    }
    return base + (e[base] <= v ? 1 : 0);
}

// -1 .. n_bins: the i with e[i] <= v < e[i + 1], where e[-1] = -inf and e[n_bins + 1] = +inf
template <bool GUESS>
__device__ __forceinline__ int bin_index(const double *e, const BinEdges &g, double v) {
    const int nb = g.n_bins;
    if (!GUESS) return bin_upper_bound(e, nb + 1, v) - 1;
    double t = (v - g.e0) * g.inv_w;
    t = fmin(fmax(t, 0.0), (double)(nb - 1));            // (fmax drops a NaN)
    int i = (int)t;
#pragma unroll
    for (int s = 0; s < BIN_FIX; s++) {
        const int ic = min(max(i, 0), nb - 1);           // (the LDS index stays in range once i has left it)
        const double a = e[ic], b = e[ic + 1];
        const int step = v < a ? -1 : (v >= b ? 1 : 0);
        i += (i >= 0 && i < nb) ? step : 0;
    }
    bool good;
    if (i < 0) good = v < e[0];
    else if (i >= nb) good = v >= e[nb];
    else good = e[i] <= v && v < e[i + 1];
    if (!good) i = bin_upper_bound(e, nb + 1, v) - 1;
    return i;
}

// lanes holding the same cell as the first pending lane add their number in one LDS atomic
__device__ __forceinline__ void bin_count(uint32_t *h, bool m, uint32_t key) {
    uint64_t todo = __ballot(m);
    const uint32_t lane = threadIdx.x & 63;
    for (int round = 0; todo && round < BIN_PEEL; round++) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint32_t k0 = __shfl(key, leader, 64);
        const uint64_t same = __ballot(m && key == k0) & todo;
        if (lane == (uint32_t)leader) atomicAdd(&h[k0], (uint32_t)__popcll(same));
        todo &= ~same;
        if (__popcll(same) < BIN_PEEL_MIN) break;       // few lanes share a code (many bins in use): the rest add on their own
    }
    if ((todo >> lane) & 1) atomicAdd(&h[key], 1u);
}

// dynamic LDS: (n_bins + 1) doubles of edges, then (COUNTS) n_bins + 2 counters
template <bool I64, bool GUESS, bool CODES, bool COUNTS>
__global__ __launch_bounds__(BIN_THREADS) void bin_kernel(BinCol c, BinEdges g, int32_t *__restrict__ codes, unsigned long long *counters) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bin_smem[];
    double *e = reinterpret_cast<double *>(bin_smem);
    uint32_t *h = reinterpret_cast<uint32_t *>(bin_smem + (size_t)(g.n_bins + 1) * 8);
    const int nb = g.n_bins;
    for (int i = threadIdx.x; i <= nb; i += BIN_THREADS) e[i] = g.edges[i];
    if (COUNTS)
        for (int i = threadIdx.x; i < nb + 2; i += BIN_THREADS) h[i] = 0;
    __syncthreads();

    const bool aligned = (reinterpret_cast<uintptr_t>(c.data) & 15) == 0;
    const bool pair_store = CODES && (reinterpret_cast<uintptr_t>(codes) & 7) == 0;
    const int64_t tiles = (c.n + BIN_TILE - 1) / BIN_TILE;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t r0 = t * BIN_TILE + 2 * (int64_t)threadIdx.x;
        uint64_t v[BIN_LOADS][2];
        uint32_t in[BIN_LOADS], nul[BIN_LOADS];
#pragma unroll
        for (int k = 0; k < BIN_LOADS; k++) {                // every load of the tile in flight before the first search
            const int64_t r = r0 + (int64_t)k * 2 * BIN_THREADS;          // even: both rows' mask bits lie in one byte
            in[k] = nul[k] = 0;
            v[k][0] = v[k][1] = 0;
            if (r + 1 < c.n) {
                if (aligned) {
                    const ulonglong2 q = *reinterpret_cast<const ulonglong2 *>(c.data + r);
                    v[k][0] = q.x; v[k][1] = q.y;
                } else {
                    v[k][0] = c.data[r]; v[k][1] = c.data[r + 1];
                }
                in[k] = 3;
            } else if (r < c.n) {
                v[k][0] = c.data[r];
                in[k] = 1;
            }
            if (c.null && in[k]) nul[k] = ((uint32_t)c.null[r >> 3] >> (r & 7)) & 3;
        }
#pragma unroll
        for (int k = 0; k < BIN_LOADS; k++) {                // (a uniform loop: the ballots of bin_count see every lane)
            const int64_t r = r0 + (int64_t)k * 2 * BIN_THREADS;
            int32_t code[2];
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const double x = I64 ? (double)(int64_t)v[k][j] : __longlong_as_double((long long)v[k][j]);
                const bool here = (in[k] >> j) & 1;
                int32_t cd = PANDRS_HIP_BIN_NAN;
                if (here && !((nul[k] >> j) & 1) && !bin_is_nan(x)) {
                    const int i = bin_index<GUESS>(e, g, x);
                    cd = i >= 0 && i < nb ? i : PANDRS_HIP_BIN_NONE;
                }
                code[j] = cd;
                if (COUNTS) bin_count(h, here, cd >= 0 ? (uint32_t)cd : (uint32_t)(nb - 1 - cd));    // NONE: nb, NAN: nb + 1
            }
            if (CODES) {
                if (in[k] == 3 && pair_store) *reinterpret_cast<int2 *>(codes + r) = make_int2(code[0], code[1]);
                else {
                    if (in[k] & 1) codes[r] = code[0];
                    if (in[k] & 2) codes[r + 1] = code[1];
                }
            }
        }
    }
    if (COUNTS) {
        __syncthreads();
        for (int i = threadIdx.x; i < nb + 2; i += BIN_THREADS)
            if (h[i]) atomicAdd(&counters[i], (unsigned long long)h[i]);
    }
}

template <bool I64, bool GUESS>
static void bin_launch(pandrs_hip_ctx *c, int grid, size_t lds, const BinCol &bc, const BinEdges &be, int32_t *codes, unsigned long long *counters,
                       bool want_counts) {
    if (codes && want_counts) hipLaunchKernelGGL((bin_kernel<I64, GUESS, true, true>), dim3(grid), dim3(BIN_THREADS), lds, c->stream, bc, be, codes, counters);
    else if (codes) hipLaunchKernelGGL((bin_kernel<I64, GUESS, true, false>), dim3(grid), dim3(BIN_THREADS), lds, c->stream, bc, be, codes, counters);
    else hipLaunchKernelGGL((bin_kernel<I64, GUESS, false, true>), dim3(grid), dim3(BIN_THREADS), lds, c->stream, bc, be, codes, counters);
}

// Whether the guess applies: at least two bins and e[0 .. n_bins) evenly spaced, every |e[i] - (e[0] + i w)| <= w / 4 for
// w = (e[n_bins - 1] - e[0]) / (n_bins - 1) finite and positive (the last edge is free: cut moves it).  The spacing decides how
// often a lane needs a correction step, never which code it ends with.
static bool bin_evenly_spaced(const double *e, int32_t n_bins, double *inv_w) {
    if (n_bins < 2) return false;
    const double w = (e[n_bins - 1] - e[0]) / (double)(n_bins - 1);
    if (!(w > 0.0) || !std::isfinite(w) || !std::isfinite(e[0]) || !std::isfinite(1.0 / w)) return false;
    for (int32_t i = 1; i < n_bins; i++)
        if (!(std::fabs(e[i] - (e[0] + (double)i * w)) <= 0.25 * w)) return false;
    *inv_w = 1.0 / w;
    return true;
}

int32_t bin_entry(pandrs_hip_ctx *c, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows, const double *edges, int32_t n_bins,
                  int32_t out_mem_space, int32_t *out_codes, int64_t *out_counts) {
    if (!c || !col || !edges || n_rows < 0 || (n_rows > 0 && !col->data) || (!out_codes && !out_counts))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "bin: bad arguments");
    ST_TRY(check_mem_space("bin", mem_space, out_codes ? out_mem_space : PANDRS_HIP_MEM_DEVICE));        // (no output, no output space)
    if (col->dtype != PANDRS_HIP_I64 && col->dtype != PANDRS_HIP_F64)
        return fail(PANDRS_HIP_ERR_TYPE_MISMATCH, "bin: the column has dtype %d, expected I64 or F64", col->dtype);
    if (n_bins < 1 || n_bins > BIN_MAX_BINS)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "bin: %d bins; one call takes 1 to %d", n_bins, BIN_MAX_BINS);
    for (int32_t i = 0; i <= n_bins; i++)
        if (edges[i] != edges[i] || (i && edges[i] < edges[i - 1]))
            return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "bin: edge %d is %g after %g; the edges must not decrease and none may be NaN", i, edges[i],
                        i ? edges[i - 1] : edges[0]);
    if (n_rows >= (int64_t(1) << 32))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "bin: %lld rows; one call takes fewer than 2^32", (long long)n_rows);
    if (reinterpret_cast<uintptr_t>(out_codes) & 3) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "bin: out_codes must be 4-byte aligned");
    const size_t n_cells = (size_t)n_bins + 2;
    if (out_counts) std::fill(out_counts, out_counts + n_cells, int64_t(0));
    if (n_rows == 0) return 0;
    const size_t code_bytes = (size_t)n_rows * 4, edge_bytes = ((size_t)n_bins + 1) * 8;
    std::lock_guard<std::mutex> lock(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    timings_begin(c);

    ColView cv{col->data, col->null_mask};
    int32_t *d_codes = out_codes;
    Stager stg{c, mem_space, out_mem_space};
    if (const size_t need = stg.col_size(*col, n_rows) + stg.out_size(out_codes, code_bytes)) {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_STAGE_IN);
        ST_TRY(stg.reserve(need));
        cv = stg.col(*col, n_rows);
        d_codes = stg.out(out_codes, code_bytes);
        if (stg.status) return stg.status;
    }
    if (reinterpret_cast<uintptr_t>(cv.data) & 7) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "bin: the column must be 8-byte aligned");
    // the workspace does not grow with n_rows: the edges and the counters
    ST_TRY(c->work.ensure(Arena::padded(edge_bytes) + Arena::padded(n_cells * 8), c->stream));
    double *d_edges = c->work.take<double>((size_t)n_bins + 1);
    unsigned long long *d_counts = c->work.take<unsigned long long>(n_cells);
    if (!d_edges || !d_counts) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (bin)");

    BinEdges be{d_edges, n_bins, edges[0], 0.0};
    const bool even = bin_evenly_spaced(edges, n_bins, &be.inv_w);
    const int64_t path = c->opt.bin_path;                // 1: always the search; 2: the guess wherever it applies; 0: by the bin count
    const bool guess = even && path != 1 && (path == 2 || n_bins >= BIN_GUESS_MIN_BINS);
    // the pinned block carries the edges out and, after the kernel, the counts back: one stream, so the copies are ordered
    static_assert((BIN_MAX_BINS + 2) * 8 <= (1 << 16), "the counts of a call fit the context's pinned block");
    std::memcpy(c->pinned, edges, edge_bytes);
    const int64_t tiles = (n_rows + BIN_TILE - 1) / BIN_TILE;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)c->n_cu * BIN_BLOCKS_PER_CU, tiles));
    const size_t lds = edge_bytes + (out_counts ? n_cells * 4 : 0);
    const BinCol bc{static_cast<const uint64_t *>(cv.data), cv.mask, n_rows};
    {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_AGGREGATE);
        HIP_TRY(hipMemcpyAsync(d_edges, c->pinned, edge_bytes, hipMemcpyHostToDevice, c->stream));
        if (out_counts) HIP_TRY(hipMemsetAsync(d_counts, 0, n_cells * 8, c->stream));
        const bool i64 = col->dtype == PANDRS_HIP_I64;
        if (i64 && guess) bin_launch<true, true>(c, grid, lds, bc, be, d_codes, d_counts, out_counts != nullptr);
        else if (i64) bin_launch<true, false>(c, grid, lds, bc, be, d_codes, d_counts, out_counts != nullptr);
        else if (guess) bin_launch<false, true>(c, grid, lds, bc, be, d_codes, d_counts, out_counts != nullptr);
        else bin_launch<false, false>(c, grid, lds, bc, be, d_codes, d_counts, out_counts != nullptr);
        HIP_TRY(hipGetLastError());
    }
    c->timings.n_partitions = guess ? 2 : 1;             // which path answered: 1 = search, 2 = guess
    c->timings.algorithmic_bytes = (int64_t)n_rows * 8 + (cv.mask ? (n_rows + 7) / 8 : 0) + (d_codes ? (int64_t)code_bytes : 0);
    ST_TRY(stg.copy_back(code_bytes));
    if (out_counts) HIP_TRY(hipMemcpyAsync(c->pinned, d_counts, n_cells * 8, hipMemcpyDeviceToHost, c->stream));
    ST_TRY(timings_end(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (out_counts) std::memcpy(out_counts, c->pinned, n_cells * 8);
    return 0;
}

}  // namespace pandrs
