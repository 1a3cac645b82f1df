// cumulative.hip — running folds and lagged differences of one numeric column in row order, behind PandasCompatExt::cumsum /
// cumprod / cummax / cummin (reference src/dataframe/pandas_compat/functions.rs:280-327), cumcount (:2081-2094), shift
// (:328-342), pct_change (:514-530) and diff (:531-541), gfx950, wave64.
//
// The scan is reduce-then-apply over contiguous spans.  The column is cut into tiles of CUM_TILE rows and the grid's workgroups
// own contiguous spans of whole tiles (span b: base + (b < rem) tiles).
// 1. Reduce.  Every workgroup folds its span into one summary.  The five folds are commutative, so a thread folds the rows it
//    loads (16 bytes per lane, CUM_LOADS loads in flight) and the workgroup folds its threads: no scan here.
// 2. Apply.  The prologue folds the summaries of the spans before its own (at most grid states, read from L2) into the carry,
//    then the span's tiles are scanned from that carry and written.  Every hand-off between workgroups is a kernel boundary, as
//    in the sort, the rank and the fill: no workgroup waits for another and nothing spins on a flag.
// A tile in registers: wave w owns rows w * 512 .. w * 512 + 511 of the tile, its load k the 128 rows from k * 128, lane l the
// rows 2l and 2l + 1 of those: one 16-byte access per lane, 1 KiB per wave instruction, loads and stores alike.  The scan runs
// in that striped order: the lane's pair, a wave scan by cross-lane moves per load, the loads chained through their lane-63
// totals, the waves through LDS with one barrier per tile (the totals are double-buffered).
// The input mask is read one byte per eight rows (lanes 0 .. 15 of a load read its 16 bytes and hand them on by a cross-lane
// move); a scan's output mask is the input mask with the bits past n_rows cleared, so the same lanes store it bytewise.
// cumprod scans (mantissa, exponent) states and converts at the end; the first row whose conversion leaves f64's range is
// recorded, and a second kernel pair, which ends at once when there is none, rewrites the rows after it from the sticky value.
// The lag kernel is one stream: a row reads x[i] and x[i - periods] and writes one cell; four lanes build one mask byte.
#include "cumulative.hpp"

#include <algorithm>

namespace pandrs {

#pragma clang fp contract(off)      // diff / pct_change are the reference's expressions, every operation rounded on its own

constexpr int CUM_THREADS = 256;                        // 4 waves
constexpr int CUM_WAVES = CUM_THREADS / 64;
constexpr int CUM_LOADS = 4;                            // 16-byte loads per lane and tile
constexpr int CUM_WAVE_ROWS = CUM_LOADS * 128;          // rows one wave owns in a tile
constexpr int CUM_TILE = CUM_WAVES * CUM_WAVE_ROWS;     // 2048 rows: cum_tile_rows of pandrs_hip.h
constexpr int CUM_BLOCKS_PER_CU = 4;                    // cum_blocks_per_cu of pandrs_hip.h
constexpr uint64_t CUM_NONE = ~0ull;                    // the excursion cell: no row left f64's range

struct CumSpans {
    int64_t tiles, base, rem;       // span b holds base + (b < rem) tiles from tile b * base + min(b, rem)
    void *summary;                  // [grid] states
    uint64_t *excursion;            // PROD: min over rows of row << 2 | sign << 1 | is_inf, CUM_NONE when there is none
};

// ---- the folds ------------------------------------------------------------------------------------------------------------
// (ProdState and CumProd, the (mantissa, exponent) product: cumulative.hpp, shared with moments.hip)

__device__ __forceinline__ ProdState cum_shfl_up(ProdState v, int d) { return ProdState{__shfl_up(v.m, d, 64), (int64_t)__shfl_up((long long)v.e, d, 64)}; }
__device__ __forceinline__ ProdState cum_shfl(ProdState v, int l) { return ProdState{__shfl(v.m, l, 64), (int64_t)__shfl((long long)v.e, l, 64)}; }

__device__ __forceinline__ double cum_mant(double v) { return v; }
__device__ __forceinline__ double cum_mant(uint32_t) { return 0.0; }
__device__ __forceinline__ double cum_mant(const ProdState &v) { return v.m; }

// ---- one tile's loads -------------------------------------------------------------------------------------------------------
// the lane's two cells of the load that starts at row r0 (even); rows at or past n read as 0
__device__ __forceinline__ void cum_load2(const CumCol &c, int64_t r0, bool full, uint64_t &a, uint64_t &b) {
    if (full && c.in16) {
        const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(c.data + r0);
        a = v.x; b = v.y;
    } else {
        a = r0 < c.n ? c.data[r0] : 0;
        b = r0 + 1 < c.n ? c.data[r0 + 1] : 0;
    }
}

// the mask byte of the 8 rows that hold row r0, bits at or past n cleared: lanes 0 .. 15 read the load's 16 bytes once, every lane
// takes its own from lane / 4.  `mine` is what lanes 0 .. 15 read (the output mask byte of a scan).
__device__ __forceinline__ uint32_t cum_mask_byte(const CumCol &c, int64_t load0, uint32_t lane, uint32_t &mine) {
    mine = 0;
    if (!c.mask) return 0;                              // (uniform)
    const int64_t byte = (load0 >> 3) + lane, left = c.n - byte * 8;
    if (lane < 16 && left > 0) mine = c.mask[byte] & (left >= 8 ? 0xFFu : (0xFFu >> (8 - left)));
    return (uint32_t)__shfl((int)mine, (int)(lane >> 2), 64);
}

template <typename OP>
__device__ __forceinline__ typename OP::S cum_block_fold(typename OP::S v, typename OP::S *lds, uint32_t tid) {
    using S = typename OP::S;
    for (int o = 1; o < 64; o <<= 1) {
        const S u = cum_shfl_up(v, o);
        if ((tid & 63) >= (uint32_t)o) v = OP::combine(u, v);
    }
    __syncthreads();                                    // lds may still be read from an earlier fold
    if ((tid & 63) == 63) lds[tid >> 6] = v;
    __syncthreads();
    S t = lds[0];
#pragma unroll
    for (int w = 1; w < CUM_WAVES; w++) t = OP::combine(t, lds[w]);
    return t;
}

// first row a rescan covers (rows before it keep what the first pass wrote), or -1: no excursion, nothing to do
__device__ __forceinline__ int64_t cum_rescan_from(const CumSpans &sp) {
    const uint64_t cell = *sp.excursion;
    return cell == CUM_NONE ? -1 : (int64_t)(cell >> 2) + 1;
}

// RESCAN (PROD only): the rows after the recorded excursion, every row before them an identity
template <typename OP, bool IS_I64, bool RESCAN>
__global__ __launch_bounds__(CUM_THREADS) void cum_reduce_kernel(CumCol c, CumSpans sp) {
    using S = typename OP::S;
    __shared__ S s_tot[CUM_WAVES];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int64_t from = 0;
    if (RESCAN && (from = cum_rescan_from(sp)) < 0) return;
    const int64_t b = blockIdx.x;
    const int64_t t0 = b * sp.base + (b < sp.rem ? b : sp.rem), t1 = t0 + sp.base + (b < sp.rem ? 1 : 0);
    S acc = OP::identity();
    for (int64_t t = t0; t < t1; t++) {
        const int64_t p0 = t * CUM_TILE;
        if (RESCAN && p0 + CUM_TILE <= from) continue;
        const bool full = p0 + CUM_TILE <= c.n;
        uint64_t a[CUM_LOADS], d[CUM_LOADS];
        uint32_t mb[CUM_LOADS];
#pragma unroll
        for (int k = 0; k < CUM_LOADS; k++) {           // every load is issued before the first is used
            const int64_t l0 = p0 + wave * CUM_WAVE_ROWS + k * 128;
            cum_load2(c, l0 + 2 * lane, full, a[k], d[k]);
            uint32_t mine;
            mb[k] = cum_mask_byte(c, l0, lane, mine);
        }
#pragma unroll
        for (int k = 0; k < CUM_LOADS; k++) {
            const int64_t r0 = p0 + wave * CUM_WAVE_ROWS + k * 128 + 2 * lane;
            const uint32_t nb = mb[k] >> ((lane & 3) * 2);
            const bool skip0 = r0 >= c.n || (nb & 1) || (RESCAN && r0 < from);
            const bool skip1 = r0 + 1 >= c.n || (nb & 2) || (RESCAN && r0 + 1 < from);
            acc = OP::combine(acc, OP::elem(cum_f64(a[k], IS_I64), skip0));
            acc = OP::combine(acc, OP::elem(cum_f64(d[k], IS_I64), skip1));
        }
    }
    acc = cum_block_fold<OP>(acc, s_tot, tid);
    if (tid == 0) static_cast<S *>(sp.summary)[b] = acc;
}

template <typename OP, bool IS_I64, bool RESCAN>
__global__ __launch_bounds__(CUM_THREADS) void cum_apply_kernel(CumCol c, CumSpans sp, CumOut o) {
    using S = typename OP::S;
    constexpr bool IS_PROD = OP::IS_PROD, IS_COUNT = OP::IS_COUNT;
    __shared__ S s_fold[CUM_WAVES];
    __shared__ S s_tot[2][CUM_WAVES];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int64_t from = 0;
    double sticky = 0.0;
    if (RESCAN) {
        if ((from = cum_rescan_from(sp)) < 0) return;
        const uint64_t cell = *sp.excursion;
        sticky = (cell & 1) ? INFINITY : 0.0;
        if (cell & 2) sticky = -sticky;
    }
    const int64_t b = blockIdx.x;
    const int64_t t0 = b * sp.base + (b < sp.rem ? b : sp.rem), t1 = t0 + sp.base + (b < sp.rem ? 1 : 0);
    if (t0 >= t1) return;                               // (uniform: an empty span)

    // ---- the carry: the summaries of the spans before this one ----
    S carry = OP::identity();
    for (int64_t j = tid; j < b; j += CUM_THREADS) carry = OP::combine(carry, static_cast<const S *>(sp.summary)[j]);
    carry = OP::combine(OP::start(), cum_block_fold<OP>(carry, s_fold, tid));

    uint32_t nulls = 0;
    uint64_t first_out = CUM_NONE;                      // PROD: this thread's first row that left f64's range
    int buf = 0;
    for (int64_t t = t0; t < t1; t++, buf ^= 1) {
        const int64_t p0 = t * CUM_TILE;
        if (RESCAN && p0 + CUM_TILE <= from) continue;  // (uniform)
        const bool full = p0 + CUM_TILE <= c.n;
        uint64_t a[CUM_LOADS], d[CUM_LOADS];
        uint32_t mb[CUM_LOADS], mine[CUM_LOADS];
#pragma unroll
        for (int k = 0; k < CUM_LOADS; k++) {           // every load is issued before the first is used
            const int64_t l0 = p0 + wave * CUM_WAVE_ROWS + k * 128;
            cum_load2(c, l0 + 2 * lane, full, a[k], d[k]);
            mb[k] = cum_mask_byte(c, l0, lane, mine[k]);
        }
        // ---- the lane's pairs, then one wave scan per load ----
        S e0[CUM_LOADS], incl[CUM_LOADS];
        bool null0[CUM_LOADS], null1[CUM_LOADS];
#pragma unroll
        for (int k = 0; k < CUM_LOADS; k++) {
            const int64_t r0 = p0 + wave * CUM_WAVE_ROWS + k * 128 + 2 * lane;
            const uint32_t nb = mb[k] >> ((lane & 3) * 2);
            null0[k] = nb & 1; null1[k] = nb & 2;
            const bool skip0 = r0 >= c.n || null0[k] || (RESCAN && r0 < from);
            const bool skip1 = r0 + 1 >= c.n || null1[k] || (RESCAN && r0 + 1 < from);
            e0[k] = OP::elem(cum_f64(a[k], IS_I64), skip0);
            incl[k] = OP::combine(e0[k], OP::elem(cum_f64(d[k], IS_I64), skip1));
        }
        S pair[CUM_LOADS];
#pragma unroll
        for (int k = 0; k < CUM_LOADS; k++) pair[k] = incl[k];
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
#pragma unroll
            for (int k = 0; k < CUM_LOADS; k++) {       // CUM_LOADS independent chains
                const S u = cum_shfl_up(incl[k], s);
                if (lane >= (uint32_t)s) incl[k] = OP::combine(u, incl[k]);
            }
        }
        // ---- the loads chained through their lane-63 totals; the waves through LDS ----
        S before[CUM_LOADS];                            // the wave's rows in front of load k
        S run = OP::identity();
#pragma unroll
        for (int k = 0; k < CUM_LOADS; k++) {
            before[k] = run;
            run = OP::combine(run, cum_shfl(incl[k], 63));
        }
        if (lane == 0) s_tot[buf][wave] = run;
        __syncthreads();                                // the one barrier of the tile: the other buffer is free by the next
        S wpre = carry, total = carry;
#pragma unroll
        for (int w = 0; w < CUM_WAVES; w++) {
            const S x = s_tot[buf][w];
            total = OP::combine(total, x);
            if ((uint32_t)w < wave) wpre = OP::combine(wpre, x);
        }
        carry = total;
        // ---- write ----
#pragma unroll
        for (int k = 0; k < CUM_LOADS; k++) {
            const int64_t l0 = p0 + wave * CUM_WAVE_ROWS + k * 128, r0 = l0 + 2 * lane;
            S ex = cum_shfl_up(incl[k], 1);
            if (lane == 0) ex = OP::identity();
            const S pre = OP::combine(OP::combine(wpre, before[k]), ex);
            const S s0 = OP::combine(pre, e0[k]), s1 = OP::combine(pre, pair[k]);
            uint64_t v0, v1;
            if (RESCAN) {
                v0 = cum_bits(sticky * cum_mant(s0));      // the mantissa alone: 0 and inf absorb
                v1 = cum_bits(sticky * cum_mant(s1));
            } else {
                v0 = OP::out(s0); v1 = OP::out(s1);
            }
            if (IS_PROD && !RESCAN) {
                const double m0 = cum_mant(s0), m1 = cum_mant(s1);
                const uint64_t a0 = v0 & 0x7FFFFFFFFFFFFFFFull, a1 = v1 & 0x7FFFFFFFFFFFFFFFull;
                const bool plain0 = m0 != 0.0 && m0 == m0 && !isinf(m0), plain1 = m1 != 0.0 && m1 == m1 && !isinf(m1);
                if (plain1 && (a1 == 0 || a1 == 0x7FF0000000000000ull) && r0 + 1 < c.n)
                    first_out = min(first_out, (uint64_t)(r0 + 1) << 2 | (v1 >> 63) << 1 | (a1 ? 1 : 0));
                if (plain0 && (a0 == 0 || a0 == 0x7FF0000000000000ull) && r0 < c.n)
                    first_out = min(first_out, (uint64_t)r0 << 2 | (v0 >> 63) << 1 | (a0 ? 1 : 0));
            }
            if (!IS_COUNT) {                            // a null row is NaN under its bit; the running count is written as it is
                if (null0[k]) v0 = CANON_NAN;
                if (null1[k]) v1 = CANON_NAN;
            }
            const bool w0 = r0 < c.n && (!RESCAN || r0 >= from), w1 = r0 + 1 < c.n && (!RESCAN || r0 + 1 >= from);
            if (w0 && w1 && o.out16) {
                ulonglong2 v;
                v.x = v0; v.y = v1;
                *reinterpret_cast<ulonglong2 *>(o.data + r0) = v;
            } else {
                if (w0) o.data[r0] = v0;
                if (w1) o.data[r0 + 1] = v1;
            }
            if (!RESCAN) {                              // the output mask word is the input's, bits past n cleared; stored bytewise
                const uint32_t ob = IS_COUNT ? 0u : mine[k];
                const int64_t byte = (l0 >> 3) + lane;
                if (o.mask && lane < 16 && byte * 8 < c.n) o.mask[byte] = (uint8_t)ob;
                nulls += __popc(ob);
            }
        }
    }
    if (!RESCAN) {
        for (int s = 32; s >= 1; s >>= 1) nulls += __shfl_down((int)nulls, s, 64);
        if (lane == 0 && nulls) atomicAdd(o.n_null, nulls);
    }
    if (IS_PROD && !RESCAN) {
        for (int s = 32; s >= 1; s >>= 1) first_out = min(first_out, (uint64_t)__shfl_down((long long)first_out, s, 64));
        if (lane == 0 && first_out != CUM_NONE) atomicMin((unsigned long long *)sp.excursion, (unsigned long long)first_out);
    }
}

// ---- lag ------------------------------------------------------------------------------------------------------------------------
struct LagRow { uint64_t v; bool gone; };               // the cell and its output bit

template <int OP, bool IS_I64>
__device__ __forceinline__ LagRow lag_row(const CumCol &c, int64_t i, int64_t periods) {
    const int64_t s = i - periods;
    if (OP == PANDRS_HIP_LAG_SHIFT) {
        if (s < 0 || s >= c.n || (c.mask && bit_at(c.mask, s))) return LagRow{CANON_NAN, true};
        return LagRow{cum_bits(cum_f64(c.data[s], IS_I64)), false};
    }
    if (s < 0) return LagRow{CANON_NAN, false};         // the reference's vec![NAN; n]: a value, not a missing row
    if (c.mask && (bit_at(c.mask, i) || bit_at(c.mask, s))) return LagRow{CANON_NAN, true};
    const double curr = cum_f64(c.data[i], IS_I64), prev = cum_f64(c.data[s], IS_I64);
    if (OP == PANDRS_HIP_LAG_DIFF) return LagRow{cum_bits(curr - prev), false};
    return LagRow{prev == 0.0 ? CANON_NAN : cum_bits((curr - prev) / prev), false};
}

template <int OP, bool IS_I64>
__global__ __launch_bounds__(CUM_THREADS) void lag_kernel(CumCol c, int64_t tiles, int64_t periods, CumOut o) {
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    uint32_t nulls = 0;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t p0 = t * CUM_TILE;
#pragma unroll
        for (int k = 0; k < CUM_LOADS; k++) {           // (a uniform loop: the cross-lane moves see every lane)
            const int64_t r0 = p0 + wave * CUM_WAVE_ROWS + k * 128 + 2 * lane;
            const bool in0 = r0 < c.n, in1 = r0 + 1 < c.n;
            LagRow x0{0, false}, x1{0, false};
            if (in0) x0 = lag_row<OP, IS_I64>(c, r0, periods);
            if (in1) x1 = lag_row<OP, IS_I64>(c, r0 + 1, periods);
            if (in1 && o.out16) {
                ulonglong2 v;
                v.x = x0.v; v.y = x1.v;
                *reinterpret_cast<ulonglong2 *>(o.data + r0) = v;
            } else {
                if (in0) o.data[r0] = x0.v;
                if (in1) o.data[r0 + 1] = x1.v;
            }
            uint32_t ob = ((x0.gone ? 1u : 0u) | (x1.gone ? 2u : 0u)) << ((lane & 3) * 2);     // four lanes make one byte
            ob |= (uint32_t)__shfl_xor((int)ob, 1, 64);
            ob |= (uint32_t)__shfl_xor((int)ob, 2, 64);
            if ((lane & 3) == 0) {
                if (o.mask && in0) o.mask[r0 >> 3] = (uint8_t)ob;
                nulls += __popc(ob);
            }
        }
    }
    for (int s = 32; s >= 1; s >>= 1) nulls += __shfl_down((int)nulls, s, 64);
    if (lane == 0 && nulls) atomicAdd(o.n_null, nulls);
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
template <typename OP, bool RESCAN>
static void cum_launch(pandrs_hip_ctx *c, int grid, bool is_i64, const CumCol &cc, const CumSpans &sp, const CumOut &co) {
    if (is_i64) {
        hipLaunchKernelGGL((cum_reduce_kernel<OP, true, RESCAN>), dim3(grid), dim3(CUM_THREADS), 0, c->stream, cc, sp);
        hipLaunchKernelGGL((cum_apply_kernel<OP, true, RESCAN>), dim3(grid), dim3(CUM_THREADS), 0, c->stream, cc, sp, co);
    } else {
        hipLaunchKernelGGL((cum_reduce_kernel<OP, false, RESCAN>), dim3(grid), dim3(CUM_THREADS), 0, c->stream, cc, sp);
        hipLaunchKernelGGL((cum_apply_kernel<OP, false, RESCAN>), dim3(grid), dim3(CUM_THREADS), 0, c->stream, cc, sp, co);
    }
}

int32_t cumulative_entry(pandrs_hip_ctx *c, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows, int32_t op, int32_t out_mem_space,
                         void *out_data, uint8_t *out_null_mask, int64_t *out_n_null) {
    if (!c || !col || n_rows < 0 || (n_rows > 0 && (!col->data || !out_data)))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "cumulative: bad arguments");
    ST_TRY(check_mem_space("cumulative", mem_space, out_mem_space));
    if (op < PANDRS_HIP_CUM_SUM || op > PANDRS_HIP_CUM_COUNT)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "cumulative: op %d is not a pandrs_hip_cum_op", op);
    const bool is_i64 = col->dtype == PANDRS_HIP_I64;
    return cum_call("cumulative", c, mem_space, col, n_rows, out_mem_space, out_data, out_null_mask, out_n_null, [&](const CumCol &cc, CumOut &co) -> int32_t {
        // ---- the counter, the excursion cell and the span summaries in one arena, sized up front ----
        const int64_t tiles = (n_rows + CUM_TILE - 1) / CUM_TILE;
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)c->n_cu * CUM_BLOCKS_PER_CU, tiles));
        ST_TRY(c->work.ensure(2 * Arena::padded(8) + Arena::padded((size_t)c->n_cu * CUM_BLOCKS_PER_CU * sizeof(ProdState)), c->stream));
        co.n_null = c->work.take<uint32_t>(1);
        CumSpans sp{tiles, tiles / grid, tiles % grid, nullptr, c->work.take<uint64_t>(1)};
        sp.summary = c->work.take<ProdState>((size_t)grid);
        if (!co.n_null || !sp.excursion || !sp.summary) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (cumulative)");
        HIP_TRY(hipMemsetAsync(co.n_null, 0, 4, c->stream));
        switch (op) {
        case PANDRS_HIP_CUM_SUM: cum_launch<CumSum, false>(c, grid, is_i64, cc, sp, co); break;
        case PANDRS_HIP_CUM_MAX: cum_launch<CumExt<true>, false>(c, grid, is_i64, cc, sp, co); break;
        case PANDRS_HIP_CUM_MIN: cum_launch<CumExt<false>, false>(c, grid, is_i64, cc, sp, co); break;
        case PANDRS_HIP_CUM_COUNT: cum_launch<CumCount, false>(c, grid, is_i64, cc, sp, co); break;
        default:
            HIP_TRY(hipMemsetAsync(sp.excursion, 0xFF, 8, c->stream));
            cum_launch<CumProd, false>(c, grid, is_i64, cc, sp, co);
            cum_launch<CumProd, true>(c, grid, is_i64, cc, sp, co);        // ends at once unless a row left f64's range
        }
        // two reads and one write of the column, the mask read twice and written once, the summaries written and read
        const int64_t nbytes = (n_rows + 7) / 8;
        c->timings.algorithmic_bytes = n_rows * 24 + (cc.mask ? 2 * nbytes : 0) + (co.mask ? nbytes : 0);
        return 0;
    });
}

template <int OP>
static void lag_launch(pandrs_hip_ctx *c, int grid, bool is_i64, const CumCol &cc, int64_t tiles, int64_t periods, const CumOut &co) {
    if (is_i64) hipLaunchKernelGGL((lag_kernel<OP, true>), dim3(grid), dim3(CUM_THREADS), 0, c->stream, cc, tiles, periods, co);
    else hipLaunchKernelGGL((lag_kernel<OP, false>), dim3(grid), dim3(CUM_THREADS), 0, c->stream, cc, tiles, periods, co);
}

int32_t lag_entry(pandrs_hip_ctx *c, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows, int32_t op, int64_t periods, int32_t out_mem_space,
                  void *out_data, uint8_t *out_null_mask, int64_t *out_n_null) {
    if (!c || !col || n_rows < 0 || (n_rows > 0 && (!col->data || !out_data)))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "lag: bad arguments");
    ST_TRY(check_mem_space("lag", mem_space, out_mem_space));
    if (op < PANDRS_HIP_LAG_SHIFT || op > PANDRS_HIP_LAG_PCT_CHANGE)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "lag: op %d is not a pandrs_hip_lag_op", op);
    if (op != PANDRS_HIP_LAG_SHIFT && periods < 0)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "lag: periods %lld is negative; only SHIFT looks ahead", (long long)periods);
    const bool is_i64 = col->dtype == PANDRS_HIP_I64;
    periods = std::max<int64_t>(-n_rows, std::min<int64_t>(n_rows, periods));      // past either end no row has a source
    return cum_call("lag", c, mem_space, col, n_rows, out_mem_space, out_data, out_null_mask, out_n_null, [&](const CumCol &cc, CumOut &co) -> int32_t {
        const int64_t tiles = (n_rows + CUM_TILE - 1) / CUM_TILE;
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)c->n_cu * CUM_BLOCKS_PER_CU, tiles));
        ST_TRY(c->work.ensure(Arena::padded(4), c->stream));
        co.n_null = c->work.take<uint32_t>(1);
        if (!co.n_null) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (lag)");
        HIP_TRY(hipMemsetAsync(co.n_null, 0, 4, c->stream));
        switch (op) {
        case PANDRS_HIP_LAG_SHIFT: lag_launch<PANDRS_HIP_LAG_SHIFT>(c, grid, is_i64, cc, tiles, periods, co); break;
        case PANDRS_HIP_LAG_DIFF: lag_launch<PANDRS_HIP_LAG_DIFF>(c, grid, is_i64, cc, tiles, periods, co); break;
        default: lag_launch<PANDRS_HIP_LAG_PCT_CHANGE>(c, grid, is_i64, cc, tiles, periods, co); break;
        }
        // one read and one write of the column (the lagged read is the same lines again), the mask read and written
        const int64_t nbytes = (n_rows + 7) / 8;
        c->timings.algorithmic_bytes = n_rows * 16 + (cc.mask ? nbytes : 0) + (co.mask ? nbytes : 0);
        return 0;
    });
}

}  // namespace pandrs
