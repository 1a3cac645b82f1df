// moments.hip — the fused sums behind the whole-column shape statistics of PandasCompatExt: skew / kurtosis (reference
// src/dataframe/pandas_compat/functions.rs:1617-1665), sem / mad / prod / cv / geometric_mean / harmonic_mean
// (helpers/aggregations.rs:8-51, :108-181), var_column / std_column (functions.rs:3571-3588), range / abs_sum (:4207-4224), zscore
// (:2284-2314) and the per-frame lists sum_all ... product_all (:934-1022, :1583-1595), gfx950, wave64.  1 to MO_MAX_COLUMNS columns
// (F64 as is, I64 `as f64`) of n_rows rows in the same launches: the grid is (workgroups, columns), blockIdx.y names the column.
// The cells that count are neither null nor NaN: every reference function here filters `!v.is_nan()`.
// 1. Sums (mo_sums_kernel<LOG, RECIP, PROD>): describe.hip's stream order (mo_stream: a thread's rows depend on row numbers only) gives
//    every workgroup its counts, sum x, sum |x| and the smallest / largest order-preserving code, and, only in the variants that
//    were asked for, sum ln x over x > 0, sum 1 / x over x != 0 and the (mantissa, exponent) product of cumulative.hpp.  ln and the
//    IEEE divide are tens of f64 instructions per row: a call that wants none of them runs the lean variant and pays for none.
// 2. Central sums (mo_central_kernel, WANT_CENTRAL only): every workgroup first folds its column's partials of step 1 in ONE fixed
//    order (mo_fold_mean), so all of them, and the finish, hold the same bits of mean = sum / count: a launch-boundary reduce without
//    a launch of its own.  One more stream then gives sum d^2, sum d^3, sum d^4 and sum |d|, d = x - mean, together: the column
//    is read twice for all central statistics, not once per statistic.
// 3. Finish (mo_finish_kernel, one workgroup per column): folds the partials in that same order and writes the structs.
// Every cross-lane and workgroup fold is ds_block_sum's shape; no float atomics anywhere, so a result is the same run to run
// and the same for a host, a device and a resident column.
#include "cumulative.hpp"
#include "describe.hpp"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace pandrs {

constexpr int MO_MAX_COLUMNS = PANDRS_HIP_MOMENTS_MAX_COLUMNS;      // pandrs_hip.h: moments_max_columns
constexpr int MO_TILE = DS_TILE;                         // pandrs_hip.h: moments_tile_rows
constexpr int MO_BLOCKS_PER_CU = 4;                      // pandrs_hip.h: moments_blocks_per_cu; grid.x = min(4 x CUs, tiles)
constexpr uint32_t MO_WANT_ALL = PANDRS_HIP_MOMENTS_WANT_CENTRAL | PANDRS_HIP_MOMENTS_WANT_LOG | PANDRS_HIP_MOMENTS_WANT_RECIP |
                                 PANDRS_HIP_MOMENTS_WANT_PROD;

struct MoCols {
    const uint64_t *data[MO_MAX_COLUMNS];
    const uint8_t *null[MO_MAX_COLUMNS];
    uint32_t i64;                                        // bit c: column c is I64
};

struct MoSums {               // one workgroup's first stream
    uint64_t count, pos, nonzero, mn, mx;                // mn / mx: order-preserving codes of the f64 values
    double sum, abs_sum, log_sum, recip_sum;
    ProdState prod;
};
struct MoCentral { double m2, m3, m4, abs_dev; };        // one workgroup's second stream

__device__ __forceinline__ DsCol mo_col(const MoCols &cs, int64_t n) {
    const int col = blockIdx.y;
    return DsCol{cs.data[col], cs.null[col], n, (int)((cs.i64 >> col) & 1u)};
}

template <bool MAXOP>
__device__ __forceinline__ uint64_t mo_block_extreme(uint64_t v, uint64_t *sh) {
    for (int o = 32; o >= 1; o >>= 1) {
        const uint64_t u = __shfl_down(v, o, 64);
        v = MAXOP ? (u > v ? u : v) : (u < v ? u : v);
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t r = sh[0];
    for (int w = 1; w < DS_THREADS / 64; w++) r = MAXOP ? (sh[w] > r ? sh[w] : r) : (sh[w] < r ? sh[w] : r);
    __syncthreads();
    return r;
}
__device__ __forceinline__ ProdState mo_block_prod(ProdState v, ProdState *sh) {
    for (int o = 32; o >= 1; o >>= 1) {
        const ProdState u{__shfl_down(v.m, o, 64), (int64_t)__shfl_down((long long)v.e, o, 64)};
        v = CumProd::combine(v, u);
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    ProdState r = sh[0];
    for (int w = 1; w < DS_THREADS / 64; w++) r = CumProd::combine(r, sh[w]);
    __syncthreads();
    return r;
}

// ds_stream's rows per thread in ds_stream's order, so the folds keep describe.hip's one order, with the loads of a full tile
// issued unconditionally: behind ds_stream's per-load bounds branches the compiler waits for each load in turn, and a stream
// that only sums is then bound by latency, not by bytes (measured: docs/EXPERIMENT_LOG.md, "Moments").  The last, partial
// tile and a column 8 bytes off a 16-byte boundary take ds_stream's guarded loads.
template <class F>
__device__ __forceinline__ void mo_stream(const DsCol &c, F &&f) {
    struct alignas(16) U2 { uint64_t x, y; };
    const bool aligned = (reinterpret_cast<uintptr_t>(c.data) & 15) == 0;
    const int64_t tiles = (c.n + DS_TILE - 1) / DS_TILE, full_tiles = aligned ? c.n / DS_TILE : 0;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t r0 = t * DS_TILE + 2 * (int64_t)threadIdx.x;
        uint64_t v[DS_LOADS][2];
        uint32_t ok[DS_LOADS];
        if (t < full_tiles) {                                // (uniform) every row of the tile exists
#pragma unroll
            for (int k = 0; k < DS_LOADS; k++) {
                const int64_t r = r0 + (int64_t)k * 2 * DS_THREADS;
                const U2 *q = reinterpret_cast<const U2 *>(c.data + r);
                v[k][0] = __builtin_nontemporal_load(&q->x);
                v[k][1] = __builtin_nontemporal_load(&q->y);
                ok[k] = c.null ? 3u & ~((uint32_t)c.null[r >> 3] >> (r & 7)) : 3u;
            }
        } else {
#pragma unroll
            for (int k = 0; k < DS_LOADS; k++) {
                const int64_t r = r0 + (int64_t)k * 2 * DS_THREADS;      // even: both rows' mask bits lie in one byte
                uint32_t in = 0;
                v[k][0] = v[k][1] = 0;
                if (r + 1 < c.n) { v[k][0] = c.data[r]; v[k][1] = c.data[r + 1]; in = 3; }
                else if (r < c.n) { v[k][0] = c.data[r]; in = 1; }
                if (c.null && in) in &= ~((uint32_t)c.null[r >> 3] >> (r & 7));
                ok[k] = in;
            }
        }
#pragma unroll
        for (int k = 0; k < DS_LOADS; k++) {
            f(v[k][0], (ok[k] & 1) != 0);
            f(v[k][1], (ok[k] & 2) != 0);
        }
    }
}

struct MoShared {
    double d[DS_THREADS / 64];
    uint64_t u[DS_THREADS / 64];
    ProdState p[DS_THREADS / 64];
};

// the workgroup's fold of per-thread sums; every field is valid in every thread
template <bool LOG, bool RECIP, bool PROD>
__device__ __forceinline__ MoSums mo_block_sums(MoSums s, MoShared &sh) {
    s.count = ds_block_count(s.count, sh.u);
    s.pos = ds_block_count(s.pos, sh.u);
    s.nonzero = ds_block_count(s.nonzero, sh.u);
    s.mn = mo_block_extreme<false>(s.mn, sh.u);
    s.mx = mo_block_extreme<true>(s.mx, sh.u);
    s.sum = ds_block_sum(s.sum, sh.d);
    s.abs_sum = ds_block_sum(s.abs_sum, sh.d);
    if (LOG) s.log_sum = ds_block_sum(s.log_sum, sh.d);
    if (RECIP) s.recip_sum = ds_block_sum(s.recip_sum, sh.d);
    if (PROD) s.prod = mo_block_prod(s.prod, sh.p);
    return s;
}

__device__ __forceinline__ MoSums mo_sums_identity() {   // Rust's Sum for f64 starts at -0.0; min / max fold from +inf / -inf
    return MoSums{0, 0, 0, enc_f64(INFINITY), enc_f64(-INFINITY), -0.0, -0.0, -0.0, -0.0, ProdState{1.0, 0}};
}

// ---- 1. sums ------------------------------------------------------------------------------------------------------------------
template <bool LOG, bool RECIP, bool PROD>
__global__ __launch_bounds__(DS_THREADS) void mo_sums_kernel(MoCols cs, int64_t n, MoSums *part) {
    __shared__ MoShared sh;
    const DsCol c = mo_col(cs, n);
    MoSums s = mo_sums_identity();
    uint32_t count = 0, pos = 0, nonzero = 0;            // a thread sees fewer than 2^32 rows
    mo_stream(c, [&](uint64_t b, bool ok) {
        if (!ok || ds_is_nan(b, c.i64)) return;
        const double x = ds_value(b, c.i64);
        const uint64_t e = enc_f64(x);
        count++;
        pos += x > 0.0 ? 1u : 0u;
        nonzero += x != 0.0 ? 1u : 0u;
        s.sum += x;
        s.abs_sum += fabs(x);
        s.mn = e < s.mn ? e : s.mn;
        s.mx = e > s.mx ? e : s.mx;
        if (LOG && x > 0.0) s.log_sum += log(x);         // aggregations.rs:110-120
        if (RECIP && x != 0.0) s.recip_sum += 1.0 / x;   // :127-137
        if (PROD) s.prod = CumProd::combine(s.prod, CumProd::norm(x, 0));
    });
    s.count = count; s.pos = pos; s.nonzero = nonzero;
    s = mo_block_sums<LOG, RECIP, PROD>(s, sh);
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// the column's (sum, count) from its n_part partials, in one order whoever asks: thread i takes partials i, i + 256, ...
__device__ __forceinline__ void mo_fold_mean(const MoSums *part, int n_part, MoShared &sh, double &sum, uint64_t &count) {
    double s = -0.0;
    uint64_t k = 0;
    for (int i = threadIdx.x; i < n_part; i += DS_THREADS) { s += part[i].sum; k += part[i].count; }
    sum = ds_block_sum(s, sh.d);
    count = ds_block_count(k, sh.u);
}

// ---- 2. central sums ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DS_THREADS) void mo_central_kernel(MoCols cs, int64_t n, const MoSums *part1, MoCentral *part2) {
    __shared__ MoShared sh;
    const DsCol c = mo_col(cs, n);
    double sum;
    uint64_t count;
    mo_fold_mean(part1 + (size_t)blockIdx.y * gridDim.x, (int)gridDim.x, sh, sum, count);
    const double mean = sum / (double)count;
    MoCentral a{-0.0, -0.0, -0.0, -0.0};
    mo_stream(c, [&](uint64_t b, bool ok) {
        if (!ok || ds_is_nan(b, c.i64)) return;
        const double d = ds_value(b, c.i64) - mean, d2 = d * d;
        a.m2 += d2;
        a.m3 += d2 * d;
        a.m4 += d2 * d2;
        a.abs_dev += fabs(d);
    });
    a.m2 = ds_block_sum(a.m2, sh.d);
    a.m3 = ds_block_sum(a.m3, sh.d);
    a.m4 = ds_block_sum(a.m4, sh.d);
    a.abs_dev = ds_block_sum(a.abs_dev, sh.d);
    if (threadIdx.x == 0) part2[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = a;
}

// ---- 3. finish --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DS_THREADS) void mo_finish_kernel(const MoSums *part1, const MoCentral *part2, int n_part, uint32_t want,
                                                               pandrs_hip_moments_stats *out) {
    __shared__ MoShared sh;
    const MoSums *p1 = part1 + (size_t)blockIdx.x * n_part;
    double sum;
    uint64_t count;
    mo_fold_mean(p1, n_part, sh, sum, count);            // the bits the central stream subtracted
    MoSums s = mo_sums_identity();
    for (int i = threadIdx.x; i < n_part; i += DS_THREADS) {
        const MoSums q = p1[i];
        s.pos += q.pos; s.nonzero += q.nonzero;
        s.mn = q.mn < s.mn ? q.mn : s.mn;
        s.mx = q.mx > s.mx ? q.mx : s.mx;
        s.abs_sum += q.abs_sum; s.log_sum += q.log_sum; s.recip_sum += q.recip_sum;
        s.prod = CumProd::combine(s.prod, q.prod);
    }
    s = mo_block_sums<true, true, true>(s, sh);
    MoCentral a{-0.0, -0.0, -0.0, -0.0};
    if (want & PANDRS_HIP_MOMENTS_WANT_CENTRAL) {        // (uniform)
        const MoCentral *p2 = part2 + (size_t)blockIdx.x * n_part;
        for (int i = threadIdx.x; i < n_part; i += DS_THREADS) { a.m2 += p2[i].m2; a.m3 += p2[i].m3; a.m4 += p2[i].m4; a.abs_dev += p2[i].abs_dev; }
        a.m2 = ds_block_sum(a.m2, sh.d);
        a.m3 = ds_block_sum(a.m3, sh.d);
        a.m4 = ds_block_sum(a.m4, sh.d);
        a.abs_dev = ds_block_sum(a.abs_dev, sh.d);
    }
    if (threadIdx.x != 0) return;
    pandrs_hip_moments_stats r;
    r.count = (int64_t)count; r.count_pos = (int64_t)s.pos; r.count_nonzero = (int64_t)s.nonzero;
    r.sum = sum; r.abs_sum = s.abs_sum;
    r.min = dec_f64(s.mn); r.max = dec_f64(s.mx);
    r.mean = sum / (double)count;
    const bool central = (want & PANDRS_HIP_MOMENTS_WANT_CENTRAL) != 0;
    r.m2 = central ? a.m2 : (double)NAN; r.m3 = central ? a.m3 : (double)NAN; r.m4 = central ? a.m4 : (double)NAN;
    r.abs_dev = central ? a.abs_dev : (double)NAN;
    r.log_sum = (want & PANDRS_HIP_MOMENTS_WANT_LOG) ? s.log_sum : (double)NAN;
    r.recip_sum = (want & PANDRS_HIP_MOMENTS_WANT_RECIP) ? s.recip_sum : (double)NAN;
    r.prod = (want & PANDRS_HIP_MOMENTS_WANT_PROD) ? CumProd::value(s.prod) : (double)NAN;
    out[blockIdx.x] = r;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
template <bool LOG, bool RECIP, bool PROD>
static void mo_launch_sums(pandrs_hip_ctx *c, dim3 grid, const MoCols &cs, int64_t n, MoSums *part) {
    hipLaunchKernelGGL((mo_sums_kernel<LOG, RECIP, PROD>), grid, dim3(DS_THREADS), 0, c->stream, cs, n, part);
}

int32_t moments_entry(pandrs_hip_ctx *c, int32_t mem_space, const pandrs_hip_column *cols, int32_t n_cols, int64_t n_rows, uint32_t want,
                      pandrs_hip_moments_stats *out) {
    if (!c || !cols || !out || n_rows < 0) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "moments: bad arguments");
    ST_TRY(check_mem_space("moments", mem_space));
    if (n_cols < 1 || n_cols > MO_MAX_COLUMNS)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "moments: %d columns; one call takes 1 to %d", n_cols, MO_MAX_COLUMNS);
    if (want & ~MO_WANT_ALL) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "moments: unknown bits 0x%x in want", want & ~MO_WANT_ALL);
    for (int i = 0; i < n_cols; i++) {
        if (cols[i].dtype != PANDRS_HIP_I64 && cols[i].dtype != PANDRS_HIP_F64)
            return fail(PANDRS_HIP_ERR_TYPE_MISMATCH, "moments: column %d has dtype %d, expected I64 or F64", i, cols[i].dtype);
        if (n_rows > 0 && !cols[i].data) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "moments: column %d has no data", i);
    }
    if (n_rows >= (int64_t(1) << 32))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "moments: %lld rows; one call takes fewer than 2^32", (long long)n_rows);
    const bool central = (want & PANDRS_HIP_MOMENTS_WANT_CENTRAL) != 0;
    if (n_rows == 0) {                                      // no cell: the folds' identities (Rust's Sum starts at -0.0), NaN mean
        for (int i = 0; i < n_cols; i++) {
            pandrs_hip_moments_stats &r = out[i];
            r.count = r.count_pos = r.count_nonzero = 0;
            r.sum = r.abs_sum = -0.0;
            r.min = INFINITY; r.max = -INFINITY;
            r.mean = NAN;
            r.m2 = r.m3 = r.m4 = r.abs_dev = central ? -0.0 : NAN;
            r.log_sum = (want & PANDRS_HIP_MOMENTS_WANT_LOG) ? -0.0 : NAN;
            r.recip_sum = (want & PANDRS_HIP_MOMENTS_WANT_RECIP) ? -0.0 : NAN;
            r.prod = (want & PANDRS_HIP_MOMENTS_WANT_PROD) ? 1.0 : NAN;
        }
        return 0;
    }
    std::lock_guard<std::mutex> lock(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    timings_begin(c);
    const int64_t n = n_rows, tiles = (n + MO_TILE - 1) / MO_TILE;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)c->n_cu * MO_BLOCKS_PER_CU, tiles));
    // the workspace holds per-(workgroup, column) partials and the results: it does not grow with n_rows
    const size_t cells = (size_t)grid * n_cols;
    ST_TRY(c->temp.ensure(Arena::padded(cells * sizeof(MoSums)) + Arena::padded(cells * sizeof(MoCentral)) +
                          Arena::padded((size_t)n_cols * sizeof(pandrs_hip_moments_stats)) + 4096, c->stream));
    MoSums *part1 = c->temp.take<MoSums>(cells);
    MoCentral *part2 = c->temp.take<MoCentral>(cells);
    pandrs_hip_moments_stats *d_out = c->temp.take<pandrs_hip_moments_stats>((size_t)n_cols);
    if (!part1 || !part2 || !d_out) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (moments)");
    MoCols cs{};
    Stager stg{c, mem_space};
    size_t need = 0, mask_bytes = 0;
    for (int i = 0; i < n_cols; i++) {
        need += stg.col_size(cols[i], n);
        mask_bytes += cols[i].null_mask ? (size_t)(n + 7) / 8 : 0;
    }
    ColView views[MO_MAX_COLUMNS];
    for (int i = 0; i < n_cols; i++) views[i] = ColView{cols[i].data, cols[i].null_mask};
    if (need) {                                             // host columns: the phase is named only when something is staged
        PhaseTimer pt(c, PANDRS_HIP_PHASE_STAGE_IN);
        ST_TRY(stg.reserve(need));
        for (int i = 0; i < n_cols; i++) views[i] = stg.col(cols[i], n);
        if (stg.status) return stg.status;
    }
    {
        for (int i = 0; i < n_cols; i++) {
            const ColView cv = views[i];
            if (reinterpret_cast<uintptr_t>(cv.data) & 7) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "moments: column %d must be 8-byte aligned", i);
            cs.data[i] = static_cast<const uint64_t *>(cv.data);
            cs.null[i] = cv.mask;
            cs.i64 |= cols[i].dtype == PANDRS_HIP_I64 ? 1u << i : 0u;
        }
    }
    static_assert(sizeof(pandrs_hip_moments_stats) * MO_MAX_COLUMNS <= (1 << 16), "the results of a call fit the context's pinned block");
    pandrs_hip_moments_stats *h_out = static_cast<pandrs_hip_moments_stats *>(c->pinned);
    const int variant = (int)((want >> 1) & 7u);            // bit 0 LOG, bit 1 RECIP, bit 2 PROD
    {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_AGGREGATE);
        const dim3 g((unsigned)grid, (unsigned)n_cols);
        switch (variant) {
        case 0: mo_launch_sums<false, false, false>(c, g, cs, n, part1); break;
        case 1: mo_launch_sums<true, false, false>(c, g, cs, n, part1); break;
        case 2: mo_launch_sums<false, true, false>(c, g, cs, n, part1); break;
        case 3: mo_launch_sums<true, true, false>(c, g, cs, n, part1); break;
        case 4: mo_launch_sums<false, false, true>(c, g, cs, n, part1); break;
        case 5: mo_launch_sums<true, false, true>(c, g, cs, n, part1); break;
        case 6: mo_launch_sums<false, true, true>(c, g, cs, n, part1); break;
        default: mo_launch_sums<true, true, true>(c, g, cs, n, part1); break;
        }
        if (central)
            hipLaunchKernelGGL(mo_central_kernel, g, dim3(DS_THREADS), 0, c->stream, cs, n, (const MoSums *)part1, part2);
        hipLaunchKernelGGL(mo_finish_kernel, dim3((unsigned)n_cols), dim3(DS_THREADS), 0, c->stream, (const MoSums *)part1, (const MoCentral *)part2,
                           grid, want, d_out);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(h_out, d_out, (size_t)n_cols * sizeof *h_out, hipMemcpyDeviceToHost, c->stream));
    c->timings.n_partitions = 1 + variant;                  // which first-stream variant ran: 1 = lean (no ln, no divide, no product)
    c->timings.table_slots = central ? 2 : 1;               // streams over the columns
    c->timings.algorithmic_bytes = (central ? 2 : 1) * ((int64_t)n * 8 * n_cols + (int64_t)mask_bytes);
    ST_TRY(timings_end(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::memcpy(out, h_out, (size_t)n_cols * sizeof *out);
    return 0;
}

}  // namespace pandrs
