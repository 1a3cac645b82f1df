// cumulative.hpp — what cumulative.hip (folds and lags in row order) and grouped.hip (the same within groups) share: the column
// and output views, the folds' operators, and the host call frame (checks, staging, the null counter).
#pragma once
#include "engine.hpp"

namespace pandrs {

struct CumCol {
    const uint64_t *data;
    const uint8_t *mask;    // null bits or nullptr
    int64_t n;
    int in16;               // data is 16-byte aligned
};

struct CumOut {
    uint64_t *data;
    uint8_t *mask;          // ceil(n / 8) bytes or nullptr
    uint32_t *n_null;       // += the bits set in the output mask (counted with or without mask)
    int out16;              // data is 16-byte aligned
};

// ---- the folds ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double cum_shfl_up(double v, int d) { return __shfl_up(v, d, 64); }
__device__ __forceinline__ uint32_t cum_shfl_up(uint32_t v, int d) { return (uint32_t)__shfl_up((int)v, d, 64); }
__device__ __forceinline__ double cum_shfl(double v, int l) { return __shfl(v, l, 64); }
__device__ __forceinline__ uint32_t cum_shfl(uint32_t v, int l) { return (uint32_t)__shfl((int)v, l, 64); }

__device__ __forceinline__ uint64_t cum_bits(double v) {
    return v != v ? CANON_NAN : (uint64_t)__double_as_longlong(v);
}

__device__ __forceinline__ double cum_f64(uint64_t v, bool is_i64) {
    return is_i64 ? (double)(int64_t)v : __longlong_as_double((long long)v);
}

struct CumSum {
    using S = double;
    static constexpr bool IS_PROD = false, IS_COUNT = false;
    __device__ static S identity() { return -0.0; }     // the exact identity of IEEE addition
    __device__ static S start() { return 0.0; }         // the reference's fold starts from +0.0
    __device__ static S combine(S a, S b) { return a + b; }
    __device__ static S elem(double x, bool null) { return null ? -0.0 : x; }
    __device__ static uint64_t out(S s) { return cum_bits(s); }
};
template <bool MAXOP>
struct CumExt {
    using S = double;
    static constexpr bool IS_PROD = false, IS_COUNT = false;
    __device__ static S identity() { return MAXOP ? -INFINITY : INFINITY; }
    __device__ static S start() { return identity(); }
    // IEEE total order on non-NaN values, -0.0 below +0.0, as pandrs_hip_window's min / max; NaN never gets here
    __device__ static S combine(S a, S b) {
        if (MAXOP) return (a > b || (a == b && !signbit(a))) ? a : b;
        return (a < b || (a == b && signbit(a))) ? a : b;
    }
    __device__ static S elem(double x, bool null) { return null || x != x ? identity() : x; }
    __device__ static uint64_t out(S s) { return (uint64_t)__double_as_longlong(s); }
};
struct CumCount {
    using S = uint32_t;                                 // fewer than 2^32 rows per call
    static constexpr bool IS_PROD = false, IS_COUNT = true;
    __device__ static S identity() { return 0; }
    __device__ static S start() { return 0; }
    __device__ static S combine(S a, S b) { return a + b; }
    __device__ static S elem(double x, bool null) { return null || x != x ? 0u : 1u; }
    __device__ static uint64_t out(S s) { return (uint64_t)s; }
};

// the state of a product (pandrs_hip_cumulative PROD, pandrs_hip_moments prod): value = m * 2^e; 0, +-inf and NaN live in m
struct ProdState { double m; int64_t e; };
struct CumProd {
    using S = ProdState;
    static constexpr bool IS_PROD = true, IS_COUNT = false;
    __device__ static S identity() { return S{1.0, 0}; }
    __device__ static S start() { return identity(); }  // the reference's fold starts from 1.0
    __device__ static S norm(double m, int64_t e) {     // 0, +-inf and NaN pass through frexp with exponent 0
        int ex = 0;
        const double f = __builtin_frexp(m, &ex);
        const bool plain = m != 0.0 && m == m && !isinf(m);
        return S{plain ? f : m, plain ? e + ex : e};
    }
    __device__ static S combine(S a, S b) { return norm(a.m * b.m, a.e + b.e); }    // |m| <= 1 on both sides: the product stays in range
    __device__ static S elem(double x, bool null) { return null ? identity() : norm(x, 0); }
    __device__ static double value(S s) {
        const int64_t e = s.e > 4096 ? 4096 : s.e < -4096 ? -4096 : s.e;
        return __builtin_ldexp(s.m, (int)e);
    }
    __device__ static uint64_t out(S s) { return cum_bits(value(s)); }
};

// ---- host -------------------------------------------------------------------------------------------------------------------------
static bool cum_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && na && nb && x < y + nb && y < x + na;
}

// what pandrs_hip_cumulative, pandrs_hip_lag and pandrs_hip_grouped share: the checks, the staging, the counter; `run` launches the kernels
template <typename RUN>
static int32_t cum_call(const char *name, pandrs_hip_ctx *c, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows, int32_t out_mem_space,
                        void *out_data, uint8_t *out_null_mask, int64_t *out_n_null, RUN run) {
    if (col->dtype != PANDRS_HIP_I64 && col->dtype != PANDRS_HIP_F64)
        return fail(PANDRS_HIP_ERR_TYPE_MISMATCH, "%s: the column has dtype %d, expected I64 or F64", name, col->dtype);
    if (n_rows >= (int64_t(1) << 32))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "%s: %lld rows; one call takes fewer than 2^32", name, (long long)n_rows);
    if (out_n_null) *out_n_null = 0;
    if (n_rows == 0) return 0;
    const size_t n = (size_t)n_rows, nbytes = (n + 7) / 8;
    if (mem_space == out_mem_space)
        for (const void *o : {(const void *)out_data, (const void *)out_null_mask})
            if (cum_overlap(o, o == out_data ? n * 8 : nbytes, col->data, n * 8) || cum_overlap(o, o == out_data ? n * 8 : nbytes, col->null_mask, nbytes))
                return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "%s: an output overlaps the column; the call cannot run in place", name);
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
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "%s: the column and out_data must be 8-byte aligned", name);

    const CumCol cc{static_cast<const uint64_t *>(cv.data), cv.mask, n_rows, (reinterpret_cast<uintptr_t>(cv.data) & 15) == 0};
    CumOut co{static_cast<uint64_t *>(d_out), d_omask, nullptr, (reinterpret_cast<uintptr_t>(d_out) & 15) == 0};
    {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_AGGREGATE);
        ST_TRY(run(cc, co));
        HIP_TRY(hipGetLastError());
    }
    ST_TRY(stg.copy_back(n * 8));
    if (stage_mask) HIP_TRY(hipMemcpyAsync(out_null_mask, d_omask, nbytes, hipMemcpyDeviceToHost, c->stream));
    uint32_t nulls = 0;
    HIP_TRY(hipMemcpyAsync(&nulls, co.n_null, 4, hipMemcpyDeviceToHost, c->stream));
    ST_TRY(timings_end(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (out_n_null) *out_n_null = (int64_t)nulls;
    return 0;
}

}  // namespace pandrs
