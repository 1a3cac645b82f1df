// window.hip — rolling, expanding and exponentially weighted window statistics behind DataFrameWindowExt::{rolling,
// expanding, ewm} (reference src/dataframe/window.rs:13-160 over src/series/window.rs: Rolling :163-345, Expanding
// :379-500, EWM :608-724), gfx950, wave64.  One numeric column (F64 as is, I64 `as f64`), null = the reference's None.
//
// 1. Rolling sum / mean / var / std (rolling_fold_kernel): the reference's left fold in row order, bit for bit.  A
//    workgroup owns RF_T consecutive outputs, each thread RF_K consecutive ones.  The union of the workgroup's windows
//    is streamed through LDS in RF_CH-value chunks (one chunk when the tile plus its w-1 halo fits), nulls staged as
//    -0.0, the exact identity of IEEE addition.  Every thread walks the union of its RF_K windows once, in ascending
//    rows, and adds each value to every accumulator whose window holds it: the head and tail of the walk select per
//    accumulator, the middle (held by all RF_K windows) adds unconditionally.  Each accumulator therefore sees the
//    reference's values in the reference's order, starting from -0.0.  Var / std walk twice: the sums give the means
//    (sum / len, as the reference), the second walk folds (x-mean)*(x-mean) of the non-null values.  The window's
//    non-null count comes from popcounts of the null mask.  `#pragma clang fp contract(off)` keeps every product and
//    sum separately rounded, as the reference computes them.
// 2. Rolling min / max / count (van Herk / Gil-Werman, O(1) per row whatever w): rows fall in blocks [b*w, (b+1)*w).
//    A segmented forward scan gives every row the min (max) and non-null count of its block up to it (P), a segmented
//    backward scan those from it to its block's end (S); a window of w rows is S[s] (+) P[e-1], and the clamped
//    windows (starting at row 0, ending at row n) are one of the two.  NaN and null cells are the fold's start value
//    +inf (-inf), so a window of only NaN gives it, as `fold(INFINITY, f64::min)` does.
// 3. Expanding (row i covers [0, i+1)) and EWM: reduce-then-scan over 4096-row tiles (ts_*_kernel), no workgroup ever
//    waits on another: every tile's summary, one workgroup scans the summaries, then every thread re-runs its 16 rows
//    from its carried-in state.  The states: a double-double sum with the count (expanding sum / mean), (count, mean,
//    M2) merged as Chan et al. do (expanding var / std), the segmented min / max of 2. with one block, and for EWM the
//    affine map y -> a*y + b of a run of rows together with what the run makes of an unstarted series (the first
//    non-null value starts it; a null row is the identity).  EWM std is a second affine scan whose coefficients come
//    from the mean series re-run from each thread's carried-in mean.  The re-run uses the reference's expressions, so
//    only the carried-in value can differ from the sequential answer.
#include "window.hpp"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace pandrs {

constexpr int RF_K = 7;                        // outputs per thread (odd: neighbouring lanes' LDS reads fall in different banks)
constexpr int RF_T = WN_THREADS * RF_K;        // outputs per workgroup (1792)
constexpr int RF_CH = 4096;                    // LDS chunk of the windows' union, values (32 KiB)
constexpr int TS_R = 16;                       // rows per thread in the scans
constexpr int TS_T = WN_THREADS * TS_R;        // rows per tile (4096)

// ---- 1. rolling sum / mean / var / std: the register-blocked row-order fold -----------------------------------------------
template <bool SEL, bool SQ>
__device__ __forceinline__ void rf_walk(const double *xs, const uint8_t *vf, int a, int b, const int (&ls)[RF_K], const int (&le)[RF_K],
                                        const double (&mean)[RF_K], double (&acc)[RF_K]) {
    for (int r = a; r < b; r++) {
        const double x = xs[r];
        const bool ok = !SQ || vf[r];
#pragma unroll
        for (int j = 0; j < RF_K; j++) {
            bool in = ok;
            if (SEL) in = in && r >= ls[j] && r < le[j];
            double t = x;
            if (SQ) {
                const double d = x - mean[j];
                t = d * d;
            }
            acc[j] += in ? t : -0.0;
        }
    }
}

template <int OP>
__global__ __launch_bounds__(WN_THREADS) void rolling_fold_kernel(WnCol col, WnGeom g, int64_t min_periods, int64_t ddof, double *out) {
    constexpr bool SQ = OP == PANDRS_HIP_WINDOW_VAR || OP == PANDRS_HIP_WINDOW_STD;
    __shared__ double xs[RF_CH];
    __shared__ uint8_t vf[SQ ? RF_CH : 1];
    const int64_t n = g.n, T0 = (int64_t)blockIdx.x * RF_T, T1 = std::min<int64_t>(T0 + RF_T, n);
    const int64_t i0 = T0 + (int64_t)threadIdx.x * RF_K;
    const int kk = i0 < n ? (int)std::min<int64_t>(RF_K, n - i0) : 0;
    int64_t s[RF_K], e[RF_K], cnt[RF_K];
    double acc[RF_K], mean[RF_K];
    int64_t S, E, tmp;
    g.bounds(T0, S, tmp);
    g.bounds(T1 - 1, tmp, E);
    int64_t nul = 0;
#pragma unroll
    for (int j = 0; j < RF_K; j++) {
        if (j < kk) g.bounds(i0 + j, s[j], e[j]);
        else s[j] = e[j] = E;                                   // no window: never selected
        // the window's non-null count: popcounts for the first, then slide by the rows that enter and leave
        if (j == 0) nul = col.nulls_in(s[0], e[0]);
        else nul += col.nulls_in(e[j - 1], e[j]) - col.nulls_in(s[j - 1], s[j]);
        cnt[j] = (e[j] - s[j]) - nul;
        acc[j] = -0.0;
        mean[j] = 0.0;
    }
    // the thread's walk: [lo, mid_lo) selects, [mid_lo, mid_hi) lies in all its windows, [mid_hi, hi) selects
    const int64_t lo = kk ? s[0] : E, hi = kk ? e[kk - 1] : E, mid_lo = kk ? s[kk - 1] : E, mid_hi = kk ? std::max(mid_lo, e[0]) : E;
    for (int pass = 0; pass < (SQ ? 2 : 1); pass++) {
        if (pass == 1) {
#pragma unroll
            for (int j = 0; j < RF_K; j++) {
                mean[j] = acc[j] / (double)cnt[j];              // series/window.rs:236: sum / len as f64
                acc[j] = -0.0;
            }
        }
        for (int64_t C = S; C < E; C += RF_CH) {
            const int len = (int)std::min<int64_t>(RF_CH, E - C);
            __syncthreads();
            for (int q = threadIdx.x; q < len; q += WN_THREADS) {
                const int64_t r = C + q;
                const bool ok = col.valid(r);
                const double x = col.x(r);
                xs[q] = (!SQ || pass == 0) && !ok ? -0.0 : x;
                if (SQ) vf[q] = ok;
            }
            __syncthreads();
            auto clip = [&](int64_t v) { return (int)(v < C ? 0 : (v > C + len ? len : v - C)); };
            int ls[RF_K], le[RF_K];
#pragma unroll
            for (int j = 0; j < RF_K; j++) {
                ls[j] = (int)std::min<int64_t>(std::max<int64_t>(s[j] - C, -1), len + 1);
                le[j] = (int)std::min<int64_t>(std::max<int64_t>(e[j] - C, -1), len + 1);
            }
            const int a = clip(lo), b = clip(mid_lo), c2 = clip(mid_hi), d = clip(hi);
            if (SQ && pass == 1) {
                rf_walk<true, true>(xs, vf, a, b, ls, le, mean, acc);
                rf_walk<false, true>(xs, vf, b, c2, ls, le, mean, acc);
                rf_walk<true, true>(xs, vf, c2, d, ls, le, mean, acc);
            } else {
                rf_walk<true, false>(xs, vf, a, b, ls, le, mean, acc);
                rf_walk<false, false>(xs, vf, b, c2, ls, le, mean, acc);
                rf_walk<true, false>(xs, vf, c2, d, ls, le, mean, acc);
            }
        }
    }
    // finalise into LDS, then store the tile's outputs in consecutive addresses
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RF_K; j++) {
        double r = NAN;
        if (j < kk && cnt[j] >= min_periods) {
            if (OP == PANDRS_HIP_WINDOW_SUM) r = acc[j];
            else if (OP == PANDRS_HIP_WINDOW_MEAN) r = acc[j] / (double)cnt[j];
            else if (cnt[j] > ddof) {                          // series/window.rs:247-249: len <= ddof -> NaN
                r = acc[j] / (double)(cnt[j] - ddof);
                if (OP == PANDRS_HIP_WINDOW_STD) r = sqrt(r);
            }
        }
        xs[threadIdx.x * RF_K + j] = r;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < (int)(T1 - T0); q += WN_THREADS) out[T0 + q] = xs[q];
}

// ---- the tile scans: reduce-then-scan, one state per thread (16 rows), tile (4096 rows) ------------------------------------
// Op: S identity(), S combine(a, b) (a before b), S local(p0, cnt) (the thread's rows folded), emit(p0, cnt, carry)
// (the thread's rows re-run from the carried-in state, outputs written).  Positions p are in scan order.
template <class Op>
__device__ typename Op::S ts_block_scan(const Op &op, typename Op::S v, typename Op::S *sh, typename Op::S *total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < WN_THREADS; o <<= 1) {
        typename Op::S u = t >= o ? sh[t - o] : v;
        __syncthreads();
        if (t >= o) sh[t] = op.combine(u, sh[t]);
        __syncthreads();
    }
    const typename Op::S ex = t ? sh[t - 1] : op.identity();
    if (total) *total = sh[WN_THREADS - 1];
    __syncthreads();
    return ex;
}

template <class Op>
__global__ __launch_bounds__(WN_THREADS) void ts_reduce_kernel(Op op, int64_t n, typename Op::S *agg) {
    __shared__ typename Op::S sh[WN_THREADS];
    const int64_t p0 = (int64_t)blockIdx.x * TS_T + (int64_t)threadIdx.x * TS_R;
    const int cnt = p0 < n ? (int)std::min<int64_t>(TS_R, n - p0) : 0;
    typename Op::S tot;
    ts_block_scan(op, cnt ? op.local(p0, cnt) : op.identity(), sh, &tot);
    if (threadIdx.x == 0) agg[blockIdx.x] = tot;
}

template <class Op>
__global__ __launch_bounds__(WN_THREADS) void ts_scan_kernel(Op op, int64_t n_tiles, const typename Op::S *agg, typename Op::S *carry) {
    __shared__ typename Op::S sh[WN_THREADS];
    const int64_t per = (n_tiles + WN_THREADS - 1) / WN_THREADS;
    const int64_t a = std::min<int64_t>(n_tiles, (int64_t)threadIdx.x * per), b = std::min<int64_t>(n_tiles, a + per);
    typename Op::S v = op.identity();
    for (int64_t k = a; k < b; k++) v = op.combine(v, agg[k]);
    typename Op::S run = ts_block_scan(op, v, sh, nullptr);
    for (int64_t k = a; k < b; k++) {
        carry[k] = run;
        run = op.combine(run, agg[k]);
    }
}

template <class Op>
__global__ __launch_bounds__(WN_THREADS) void ts_apply_kernel(Op op, int64_t n, const typename Op::S *carry) {
    __shared__ typename Op::S sh[WN_THREADS];
    const int64_t p0 = (int64_t)blockIdx.x * TS_T + (int64_t)threadIdx.x * TS_R;
    const int cnt = p0 < n ? (int)std::min<int64_t>(TS_R, n - p0) : 0;
    const typename Op::S ex = ts_block_scan(op, cnt ? op.local(p0, cnt) : op.identity(), sh, nullptr);
    if (cnt) op.emit(p0, cnt, op.combine(carry[blockIdx.x], ex));
}

template <class Op>
int32_t ts_run(pandrs_hip_ctx *c, const Op &op, int64_t n, void *agg_mem, void *carry_mem) {
    using S = typename Op::S;
    const int64_t nt = (n + TS_T - 1) / TS_T;
    S *agg = static_cast<S *>(agg_mem), *carry = static_cast<S *>(carry_mem);
    hipLaunchKernelGGL(ts_reduce_kernel<Op>, dim3((unsigned)nt), dim3(WN_THREADS), 0, c->stream, op, n, agg);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ts_scan_kernel<Op>, dim3(1), dim3(WN_THREADS), 0, c->stream, op, nt, (const S *)agg, carry);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ts_apply_kernel<Op>, dim3((unsigned)nt), dim3(WN_THREADS), 0, c->stream, op, n, (const S *)carry);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- 2. segmented min / max with the non-null count (van Herk P / S; expanding min / max / count) -------------------------
struct VhS {
    double v;
    uint32_t f, c;     // f: the run holds a block start (in scan order); c: non-null rows since it
};

template <int MAXOP>
struct VhOp {
    using S = VhS;
    WnCol col;
    int64_t n, w;
    int back;                  // 1: scan from row n-1 down (S), block starts at each block's last row and at row n-1
    double *pv;                // per-row result (rolling), or
    uint32_t *pc;              //   its count (only when the column has nulls)
    double *out;               // expanding: the final output instead
    int64_t mp;
    int count_op;
    // IEEE total order on non-NaN values: -0.0 < +0.0; NaN never gets here
    __device__ static double pick(double a, double b) {
        if (MAXOP) return (a > b || (a == b && !signbit(a))) ? a : b;
        return (a < b || (a == b && signbit(a))) ? a : b;
    }
    __device__ static double start() { return MAXOP ? -INFINITY : INFINITY; }
    __device__ S identity() const { return S{start(), 0u, 0u}; }
    __device__ S combine(const S &a, const S &b) const { return b.f ? b : S{pick(a.v, b.v), a.f, a.c + b.c}; }
    __device__ __forceinline__ S elem(int64_t i, bool first) const {
        const bool ok = col.valid(i);
        const double x = col.x(i);
        return S{ok && !isnan(x) ? x : start(), first ? 1u : 0u, ok ? 1u : 0u};
    }
    // the rows of positions p0 .. p0+cnt-1, with their block-start flags, folded into `st` in scan order
    template <bool EMIT>
    __device__ __forceinline__ S run(int64_t p0, int cnt, S st) const {
        int64_t i = back ? n - 1 - p0 : p0;
        int64_t rem = i % w;
        for (int k = 0; k < cnt; k++) {
            const bool first = back ? (rem == w - 1 || i == n - 1) : rem == 0;
            st = combine(st, elem(i, first));
            if (EMIT) {
                if (out) out[i] = count_op ? ((int64_t)st.c >= mp ? (double)st.c : 0.0) : ((int64_t)st.c >= mp ? st.v : (double)NAN);
                else {
                    pv[i] = st.v;
                    if (pc) pc[i] = st.c;
                }
            }
            if (back) { i--; rem = rem ? rem - 1 : w - 1; }
            else { i++; rem = rem + 1 == w ? 0 : rem + 1; }
        }
        return st;
    }
    __device__ S local(int64_t p0, int cnt) const { return run<false>(p0, cnt, identity()); }
    __device__ void emit(int64_t p0, int cnt, S carry) const { run<true>(p0, cnt, carry); }
};

template <int MAXOP>
__global__ __launch_bounds__(WN_THREADS) void vh_final_kernel(WnGeom g, const double *P, const double *Sx, const uint32_t *Pc,
                                                               const uint32_t *Sc, int64_t mp, int count_op, double *out) {
    const int64_t i = (int64_t)blockIdx.x * WN_THREADS + threadIdx.x;
    if (i >= g.n) return;
    int64_t s, e;
    g.bounds(i, s, e);
    const int64_t bs = s / g.w, be = (e - 1) / g.w;
    double v;
    int64_t c;
    if (bs == be) {                       // one block: the window starts it (P) or runs to row n (S)
        if (s == bs * g.w) { v = P[e - 1]; c = Pc ? (int64_t)Pc[e - 1] : e - s; }
        else { v = Sx[s]; c = Sc ? (int64_t)Sc[s] : e - s; }
    } else {                              // e - s <= w: two neighbouring blocks
        v = VhOp<MAXOP>::pick(Sx[s], P[e - 1]);
        c = Pc ? (int64_t)Sc[s] + (int64_t)Pc[e - 1] : e - s;
    }
    out[i] = count_op ? (c >= mp ? (double)c : 0.0) : (c >= mp ? v : (double)NAN);
}

// ---- 3a. expanding sum / mean: double-double prefix with the count -----------------------------------------------------------
struct DdS {
    double hi, lo;
    int64_t c;
};

__device__ __forceinline__ void dd_add(double ah, double al, double bh, double bl, double &h, double &l) {
    const double s = ah + bh;
    if (!isfinite(s)) { h = s; l = 0.0; return; }       // +-inf / NaN: the plain sum is the reference's
    const double bb = s - ah;
    double e = (ah - (s - bb)) + (bh - bb);              // two-sum
    e = e + (al + bl);
    if (e == 0.0) { h = s; l = 0.0; return; }            // keeps the sign of a sum of zeros (-0.0 + -0.0 = -0.0)
    h = s + e;
    l = isfinite(h) ? e - (h - s) : 0.0;
}

struct DdOp {
    using S = DdS;
    WnCol col;
    int64_t mp;
    int mean;
    double *out;
    __device__ S identity() const { return S{-0.0, 0.0, 0}; }     // Rust's Sum for f64 starts at -0.0
    __device__ S combine(const S &a, const S &b) const {
        S r;
        dd_add(a.hi, a.lo, b.hi, b.lo, r.hi, r.lo);
        r.c = a.c + b.c;
        return r;
    }
    __device__ __forceinline__ S elem(int64_t i) const { return col.valid(i) ? S{col.x(i), 0.0, 1} : identity(); }
    __device__ S local(int64_t p0, int cnt) const {
        S st = identity();
        for (int k = 0; k < cnt; k++) st = combine(st, elem(p0 + k));
        return st;
    }
    __device__ void emit(int64_t p0, int cnt, S st) const {
        for (int k = 0; k < cnt; k++) {
            st = combine(st, elem(p0 + k));
            const double sum = st.lo == 0.0 ? st.hi : st.hi + st.lo;
            out[p0 + k] = st.c >= mp ? (mean ? sum / (double)st.c : sum) : (double)NAN;
        }
    }
};

// ---- 3b. expanding var / std: (count, mean, M2), merged as Chan et al. -----------------------------------------------------
struct WfS {
    double mean, m2;
    int64_t c;
};

struct WfOp {
    using S = WfS;
    WnCol col;
    int64_t mp, ddof;
    int sd;
    double *out;
    __device__ S identity() const { return S{0.0, 0.0, 0}; }
    __device__ S combine(const S &a, const S &b) const {
        if (!a.c) return b;
        if (!b.c) return a;
        const int64_t c = a.c + b.c;
        const double d = b.mean - a.mean;
        return S{a.mean + d * ((double)b.c / (double)c), a.m2 + b.m2 + d * d * ((double)a.c * (double)b.c / (double)c), c};
    }
    __device__ __forceinline__ S elem(int64_t i) const { return col.valid(i) ? S{col.x(i), 0.0, 1} : identity(); }
    __device__ S local(int64_t p0, int cnt) const {
        S st = identity();
        for (int k = 0; k < cnt; k++) st = combine(st, elem(p0 + k));
        return st;
    }
    __device__ void emit(int64_t p0, int cnt, S st) const {
        for (int k = 0; k < cnt; k++) {
            st = combine(st, elem(p0 + k));
            double r = NAN;
            // a non-finite mean means an inf or NaN value: the reference's (x - mean) is NaN for it
            if (st.c >= mp && st.c > ddof && isfinite(st.mean)) {
                r = st.m2 / (double)(st.c - ddof);
                if (sd) r = sqrt(r);
            }
            out[p0 + k] = r;
        }
    }
};

// ---- 3c. EWM: affine maps y -> a*y + b, and what a run makes of an unstarted series (f: it holds a value, y0: the result) -
struct AfS {
    double a, b, y0;
    int f;
};

__device__ __forceinline__ AfS af_combine(const AfS &A, const AfS &B) {
    return AfS{B.a * A.a, B.a * A.b + B.b, A.f ? B.a * A.y0 + B.b : B.y0, A.f | B.f};
}

// the mean (series/window.rs:640-671): NaN before the first value, which is output as itself, then
// y = alpha*v + (1-alpha)*y; a null row repeats y.  tc != NULL: only the threads' carried-in (y, started) are kept.
struct EwmMeanOp {
    using S = AfS;
    WnCol col;
    double alpha;
    double *out;
    double2 *tc;
    __device__ S identity() const { return S{1.0, -0.0, -0.0, 0}; }
    __device__ S combine(const S &a, const S &b) const { return af_combine(a, b); }
    __device__ S local(int64_t p0, int cnt) const {
        S st = identity();
        for (int k = 0; k < cnt; k++) {
            const int64_t i = p0 + k;
            if (col.valid(i)) {
                const double v = col.x(i);
                st = af_combine(st, S{1.0 - alpha, alpha * v, v, 1});
            }
        }
        return st;
    }
    __device__ void emit(int64_t p0, int cnt, S st) const {
        if (tc) { tc[p0 / TS_R] = make_double2(st.y0, st.f ? 1.0 : 0.0); return; }
        bool started = st.f;
        double y = st.y0;
        for (int k = 0; k < cnt; k++) {
            const int64_t i = p0 + k;
            if (col.valid(i)) {
                const double v = col.x(i);
                if (!started) { y = v; started = true; }
                else y = alpha * v + (1.0 - alpha) * y;
            }
            out[i] = started ? y : (double)NAN;
        }
    }
};

// std (series/window.rs:674-712): NaN up to and including the first value; then with diff = v - mean_prev,
// var = (1-alpha)*(var + alpha*diff*diff), output sqrt(var); a null row repeats it.  var (:715-724) = that output squared.
struct EwmVarOp {
    using S = AfS;
    WnCol col;
    double alpha;
    const double2 *tc;         // each thread's carried-in mean (y, started) from EwmMeanOp
    double *out;
    int var_out;
    __device__ S identity() const { return S{1.0, -0.0, -0.0, 0}; }
    __device__ S combine(const S &a, const S &b) const { return af_combine(a, b); }
    __device__ S local(int64_t p0, int cnt) const {
        const double2 m = tc[p0 / TS_R];
        double y = m.x;
        bool started = m.y != 0.0;
        S st = identity();
        for (int k = 0; k < cnt; k++) {
            const int64_t i = p0 + k;
            if (!col.valid(i)) continue;
            const double v = col.x(i);
            if (!started) {                                   // the series' first value: var starts at 0
                y = v;
                started = true;
                st = af_combine(st, S{1.0 - alpha, 0.0, 0.0, 1});
            } else {
                const double diff = v - y;
                st = af_combine(st, S{1.0 - alpha, (1.0 - alpha) * (alpha * diff * diff), 0.0, 1});
                y = alpha * v + (1.0 - alpha) * y;
            }
        }
        return st;
    }
    __device__ void emit(int64_t p0, int cnt, S st) const {
        const double2 m = tc[p0 / TS_R];
        double y = m.x, var = st.y0;
        bool started = m.y != 0.0;
        for (int k = 0; k < cnt; k++) {
            const int64_t i = p0 + k;
            double r = NAN;
            if (col.valid(i)) {
                const double v = col.x(i);
                if (!started) {
                    y = v;
                    var = 0.0;
                    started = true;
                } else {
                    const double prev_mean = y;
                    y = alpha * v + (1.0 - alpha) * prev_mean;
                    const double diff = v - prev_mean;
                    var = (1.0 - alpha) * (var + alpha * diff * diff);
                    r = sqrt(var);
                }
            } else if (started) {
                r = sqrt(var);
            }
            if (var_out) r = isnan(r) ? r : r * r;
            out[i] = r;
        }
    }
};

// ---- host side ------------------------------------------------------------------------------------------------------------
namespace {

bool op_ok(const pandrs_hip_window_spec &s) {
    if (s.kind == PANDRS_HIP_WINDOW_KIND_EWM)
        return s.op == PANDRS_HIP_WINDOW_MEAN || s.op == PANDRS_HIP_WINDOW_STD || s.op == PANDRS_HIP_WINDOW_VAR;
    return s.op >= PANDRS_HIP_WINDOW_SUM && s.op <= PANDRS_HIP_WINDOW_COUNT;
}

struct WnPlan {
    size_t rows_f64 = 0, rows_u32 = 0, tile_states = 0, thread_states = 0;
};

WnPlan plan_of(const pandrs_hip_window_spec &s, int64_t n, bool has_null) {
    WnPlan p;
    const size_t tiles = (size_t)(n + TS_T - 1) / TS_T + 1;
    const bool vh = s.kind == PANDRS_HIP_WINDOW_KIND_ROLLING &&
                    (s.op == PANDRS_HIP_WINDOW_MIN || s.op == PANDRS_HIP_WINDOW_MAX || s.op == PANDRS_HIP_WINDOW_COUNT);
    if (vh) {
        p.rows_f64 = 2;
        p.rows_u32 = has_null ? 2 : 0;
    }
    if (s.kind != PANDRS_HIP_WINDOW_KIND_ROLLING) p.tile_states = 2 * tiles;
    if (vh) p.tile_states = 4 * tiles;
    if (s.kind == PANDRS_HIP_WINDOW_KIND_EWM && s.op != PANDRS_HIP_WINDOW_MEAN) {
        p.tile_states = 4 * tiles;
        p.thread_states = (size_t)(n + TS_R - 1) / TS_R + 1;
    }
    return p;
}

}  // namespace

size_t window_workspace_bytes(const pandrs_hip_window_spec &s, int64_t n, bool has_null) {
    const WnPlan p = plan_of(s, n, has_null);
    return p.rows_f64 * Arena::padded((size_t)n * 8 + 16) + p.rows_u32 * Arena::padded((size_t)n * 4 + 16) +
           p.tile_states * 32 + Arena::padded(p.thread_states * 16) + 8 * 256 + 4096;
}

int32_t window_entry(pandrs_hip_ctx *c, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows,
                     const pandrs_hip_window_spec *spec, int32_t out_mem_space, double *out) {
    if (!c || !col || !spec || n_rows < 0 || (n_rows > 0 && (!col->data || !out)))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "window: bad arguments");
    ST_TRY(check_mem_space("window", mem_space, out_mem_space));
    if (col->dtype != PANDRS_HIP_I64 && col->dtype != PANDRS_HIP_F64)
        return fail(PANDRS_HIP_ERR_TYPE_MISMATCH, "window: the column has dtype %d, expected I64 or F64", col->dtype);
    const pandrs_hip_window_spec sp = *spec;
    if (sp.kind < PANDRS_HIP_WINDOW_KIND_ROLLING || sp.kind > PANDRS_HIP_WINDOW_KIND_EWM || !op_ok(sp))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "window: kind %d does not take op %d", sp.kind, sp.op);
    if (sp.kind == PANDRS_HIP_WINDOW_KIND_ROLLING && (sp.window < 1 || (sp.center != 0 && sp.center != 1)))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "window: window_size %lld (must be >= 1), center %d", (long long)sp.window, sp.center);
    if (sp.kind == PANDRS_HIP_WINDOW_KIND_EXPANDING && sp.min_periods < 0)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "window: expanding min_periods %lld < 0", (long long)sp.min_periods);
    if (sp.kind != PANDRS_HIP_WINDOW_KIND_EWM && sp.ddof < 0)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "window: ddof %lld < 0", (long long)sp.ddof);
    if (sp.kind == PANDRS_HIP_WINDOW_KIND_EWM && !std::isfinite(sp.alpha))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "window: EWM alpha is not finite");
    if (n_rows >= (int64_t(1) << 32))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "window: %lld rows; one call takes fewer than 2^32", (long long)n_rows);
    std::lock_guard<std::mutex> lock(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    timings_begin(c);
    if (n_rows == 0) return timings_end(c);
    const int64_t n = n_rows;
    const size_t dbytes = (size_t)n * 8, mbytes = (size_t)(n + 7) / 8;
    const bool has_null = col->null_mask != nullptr;
    // ---- every buffer sized up front ----
    ST_TRY(c->win.ensure(window_workspace_bytes(sp, n, has_null), c->stream));
    ColView cv{col->data, col->null_mask};
    double *d_out = out;
    Stager stg{c, mem_space, out_mem_space};
    if (const size_t need = stg.col_size(*col, n) + stg.out_size(out, dbytes)) {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_STAGE_IN);
        ST_TRY(stg.reserve(need));
        cv = stg.col(*col, n);
        d_out = stg.out(out, dbytes);
        if (stg.status) return stg.status;
    }
    const void *d_data = cv.data;
    const uint8_t *d_null = cv.mask;
    if (reinterpret_cast<uintptr_t>(d_data) & 7) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "window: the column must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_out) & 7) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "window: the output must be 8-byte aligned");
    const WnPlan plan = plan_of(sp, n, has_null);
    double *rows0 = plan.rows_f64 ? c->win.take<double>((size_t)n + 2) : nullptr;
    double *rows1 = plan.rows_f64 ? c->win.take<double>((size_t)n + 2) : nullptr;
    uint32_t *cnt0 = plan.rows_u32 ? c->win.take<uint32_t>((size_t)n + 4) : nullptr;
    uint32_t *cnt1 = plan.rows_u32 ? c->win.take<uint32_t>((size_t)n + 4) : nullptr;
    const size_t tiles = (size_t)(n + TS_T - 1) / TS_T + 1;
    char *ts = plan.tile_states ? c->win.take<char>(plan.tile_states * 32) : nullptr;
    double2 *tc = plan.thread_states ? c->win.take<double2>(plan.thread_states) : nullptr;
    if ((plan.rows_f64 && (!rows0 || !rows1)) || (plan.rows_u32 && (!cnt0 || !cnt1)) || (plan.tile_states && !ts) ||
        (plan.thread_states && !tc))
        return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (window)");
    char *agg0 = ts, *car0 = ts ? ts + tiles * 32 : nullptr;
    char *agg1 = ts && plan.tile_states >= 4 * tiles ? ts + 2 * tiles * 32 : nullptr, *car1 = agg1 ? agg1 + tiles * 32 : nullptr;

    const WnCol wc{d_data, d_null, n, (int64_t)mbytes, col->dtype == PANDRS_HIP_I64 ? 1 : 0};
    {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_OTHER);
        if (sp.kind == PANDRS_HIP_WINDOW_KIND_ROLLING) {
            const int64_t w = std::min<int64_t>(sp.window, 2 * n + 2);
            const WnGeom g{n, w, w / 2, sp.center};
            const int64_t mp = sp.min_periods < 0 ? sp.window : sp.min_periods;   // series/window.rs:146
            if (sp.op <= PANDRS_HIP_WINDOW_STD) {
                const dim3 grid((unsigned)((n + RF_T - 1) / RF_T)), block(WN_THREADS);
                switch (sp.op) {
                case PANDRS_HIP_WINDOW_SUM: hipLaunchKernelGGL(rolling_fold_kernel<PANDRS_HIP_WINDOW_SUM>, grid, block, 0, c->stream, wc, g, mp, sp.ddof, d_out); break;
                case PANDRS_HIP_WINDOW_MEAN: hipLaunchKernelGGL(rolling_fold_kernel<PANDRS_HIP_WINDOW_MEAN>, grid, block, 0, c->stream, wc, g, mp, sp.ddof, d_out); break;
                case PANDRS_HIP_WINDOW_VAR: hipLaunchKernelGGL(rolling_fold_kernel<PANDRS_HIP_WINDOW_VAR>, grid, block, 0, c->stream, wc, g, mp, sp.ddof, d_out); break;
                default: hipLaunchKernelGGL(rolling_fold_kernel<PANDRS_HIP_WINDOW_STD>, grid, block, 0, c->stream, wc, g, mp, sp.ddof, d_out); break;
                }
                HIP_TRY(hipGetLastError());
            } else {
                const int count_op = sp.op == PANDRS_HIP_WINDOW_COUNT;
                const dim3 grid((unsigned)((n + WN_THREADS - 1) / WN_THREADS)), block(WN_THREADS);
                if (sp.op == PANDRS_HIP_WINDOW_MAX) {
                    ST_TRY(ts_run(c, VhOp<1>{wc, n, w, 0, rows0, cnt0, nullptr, 0, 0}, n, agg0, car0));
                    ST_TRY(ts_run(c, VhOp<1>{wc, n, w, 1, rows1, cnt1, nullptr, 0, 0}, n, agg1, car1));
                    hipLaunchKernelGGL(vh_final_kernel<1>, grid, block, 0, c->stream, g, rows0, rows1, cnt0, cnt1, mp, 0, d_out);
                } else {
                    ST_TRY(ts_run(c, VhOp<0>{wc, n, w, 0, rows0, cnt0, nullptr, 0, 0}, n, agg0, car0));
                    ST_TRY(ts_run(c, VhOp<0>{wc, n, w, 1, rows1, cnt1, nullptr, 0, 0}, n, agg1, car1));
                    hipLaunchKernelGGL(vh_final_kernel<0>, grid, block, 0, c->stream, g, rows0, rows1, cnt0, cnt1, mp, count_op, d_out);
                }
                HIP_TRY(hipGetLastError());
            }
        } else if (sp.kind == PANDRS_HIP_WINDOW_KIND_EXPANDING) {
            const int64_t mp = sp.min_periods;
            switch (sp.op) {
            case PANDRS_HIP_WINDOW_SUM:
            case PANDRS_HIP_WINDOW_MEAN:
                ST_TRY(ts_run(c, DdOp{wc, mp, sp.op == PANDRS_HIP_WINDOW_MEAN, d_out}, n, agg0, car0));
                break;
            case PANDRS_HIP_WINDOW_VAR:
            case PANDRS_HIP_WINDOW_STD:
                ST_TRY(ts_run(c, WfOp{wc, mp, sp.ddof, sp.op == PANDRS_HIP_WINDOW_STD, d_out}, n, agg0, car0));
                break;
            case PANDRS_HIP_WINDOW_MAX:
                ST_TRY(ts_run(c, VhOp<1>{wc, n, n, 0, nullptr, nullptr, d_out, mp, 0}, n, agg0, car0));
                break;
            default:
                ST_TRY(ts_run(c, VhOp<0>{wc, n, n, 0, nullptr, nullptr, d_out, mp, sp.op == PANDRS_HIP_WINDOW_COUNT}, n, agg0, car0));
                break;
            }
        } else if (sp.op == PANDRS_HIP_WINDOW_MEAN) {
            ST_TRY(ts_run(c, EwmMeanOp{wc, sp.alpha, d_out, nullptr}, n, agg0, car0));
        } else {
            ST_TRY(ts_run(c, EwmMeanOp{wc, sp.alpha, nullptr, tc}, n, agg0, car0));
            ST_TRY(ts_run(c, EwmVarOp{wc, sp.alpha, tc, d_out, sp.op == PANDRS_HIP_WINDOW_VAR}, n, agg1, car1));
        }
    }
    ST_TRY(stg.copy_back(dbytes));
    c->timings.algorithmic_bytes = 2 * (int64_t)dbytes + (has_null ? (int64_t)mbytes : 0);     // the column (+ mask) in, the result out
    ST_TRY(timings_end(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace pandrs
