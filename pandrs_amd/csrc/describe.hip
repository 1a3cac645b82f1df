// describe.hip — count / mean / std / min / quartiles / max of one numeric column, and exact percentiles, behind
// OptimizedDataFrame::describe / describe_all (reference src/optimized/split_dataframe/stats.rs:50-171 over
// src/stats/descriptive.rs:91-200), gfx950, wave64.  One column (F64 as is, I64 `as f64`), null = the reference's None.
//
// No sort and no per-row workspace: the order statistics come from a multi-rank MSD radix SELECT over the whole column.
// Every hand-off between workgroups is a kernel boundary, and nothing returns to the host before the results do.
// 1. Moments (ds_moments_kernel): one stream of 16-byte loads over the column and its null mask gives every workgroup's
//    non-null and NaN counts, sum, and smallest / largest order-preserving code (enc_f64 / enc_i64) of its numbers.
// 2. Ranks (ds_ranks_kernel, one workgroup): reduces those in a fixed order, evaluates the reference's
//    `index = (p / 100.0) * (n - 1) as f64`, floor and ceil for every requested percentile in double, and keeps the distinct
//    target ranks ascending ("slots").  A rank inside the trailing NaN block is NaN without a search.  The selection
//    works on d = code - min_code, whose width decides the number of 8-bit digit passes (0: every number is equal).
// 3. Selection, most significant digit first (ds_select_kernel + ds_pick_kernel per digit): every pass streams the column
//    and matches d's bits above the digit against the live prefixes ("groups"; slots that still share a prefix share one).
//    A matching row counts its digit in the workgroup's LDS histogram, equal (group, digit) pairs of a wave first folded by
//    ballot so that a column of few distinct values does not serialise on one LDS address; the non-zero bins are added to
//    the global counts.  One workgroup then scans each group's 256 counts and narrows every slot to its digit and its rank
//    within that bin.  The first pass also accumulates sum (x - mean)^2, so std costs no stream of its own.
//    The host enqueues all eight passes; a pass beyond the width returns at once.
// 4. Finish (one thread): decodes the selected codes (I64: the selected integer `as f64`), interpolates with the reference's
//    expression, FMA contraction off, and writes the results where the entry's one copy picks them up.
// 5. Ranks by number (pandrs_hip_bin_edges): a request may name integer ranks among the cells that are neither null nor NaN
//    instead of percentiles: QCUT(q) asks for min((uint64)((double)m * (double)i / (double)q), m - 1), i = i0 .. i0 + n, m the
//    count of those cells, known in step 2.  Up to DS_MAX_SLOTS ranks per selection, every weight zero: ds_finish_ranks_kernel
//    returns the decoded elements with min, max and m.  CUT needs min and max only: steps 1 and 2, no selection.
#include "describe.hpp"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace pandrs {

// (DS_THREADS, DS_LOADS, DS_TILE, DS_BLOCKS_PER_CU, the column view and the stream: describe.hpp)
constexpr int DS_MAX_P = 16;                             // percentiles per call
constexpr int DS_MAX_SLOTS = 2 * DS_MAX_P;               // distinct target ranks (lo and hi of each)
constexpr int DS_MAX_OS = 8;                             // order statistics per call, two ranks each at the most
static_assert(2 * DS_MAX_OS <= DS_MAX_SLOTS, "the ranks of one order-statistics call fit the selection's slots");
constexpr int DS_DIGIT = 8, DS_BINS = 1 << DS_DIGIT;
constexpr int DS_MAX_PASSES = 64 / DS_DIGIT;
constexpr int DS_PEEL = 4;                               // (group, digit) pairs a wave folds by ballot before plain atomics

struct DsReq {
    double p[DS_MAX_P];
    int32_t n_p;
    int32_t rank_q, rank_i0, rank_n;      // ranks by number: QCUT(rank_q)'s ranks i0 .. i0 + rank_n (rank_n <= DS_MAX_SLOTS; n_p is 0 then)
    int32_t n_os;                         // order statistics by the reference's index rules (n_p and rank_n are 0 then)
    int32_t os_op[DS_MAX_OS];             // pandrs_hip_order_stat, or -1: the host has answered NaN (an argument the reference refuses)
    double os_arg[DS_MAX_OS];
};

struct DsPart {               // one workgroup's moments
    double sum;
    uint64_t nn, nan, mn, mx;
};

struct DsState {
    uint64_t nn, nan, mn, mx;             // non-null cells, NaN cells among them, extreme codes of the numbers
    double sum, mean, ssq;
    uint64_t vary;                        // OR of d over the numbers, known after the first digit stream
    int32_t n_pass, n_slots, n_groups, pad;
    int32_t p_lo[DS_MAX_P], p_hi[DS_MAX_P];   // slot of each percentile's lower / upper rank
    double p_w[DS_MAX_P];                 // index - lower_index
    uint64_t s_rank[DS_MAX_SLOTS];        // the slot's rank among its group's rows
    int32_t s_group[DS_MAX_SLOTS];        // -1: the rank lies in the NaN block
    uint64_t g_prefix[DS_MAX_SLOTS];      // the digits of d chosen so far
    int32_t r_slot[DS_MAX_SLOTS];         // ranks by number: the slot of each requested rank
    int32_t o_lo[DS_MAX_OS], o_hi[DS_MAX_OS];   // order statistics: the slots of the op's one or two ranks, -1 = none (the result is NaN)
    uint64_t o_t[DS_MAX_OS];              // TRIMMED_MEAN: t, the cells cut from either end
};

// (sum, nn, nan, mn, mx) over the workgroup; the result is valid in thread 0
__device__ __forceinline__ DsPart ds_block_part(DsPart p, double *shd, uint64_t *shu) {
    for (int o = 32; o >= 1; o >>= 1) {
        p.nn += __shfl_down(p.nn, o, 64);
        p.nan += __shfl_down(p.nan, o, 64);
        const uint64_t a = __shfl_down(p.mn, o, 64), b = __shfl_down(p.mx, o, 64);
        p.mn = a < p.mn ? a : p.mn;
        p.mx = b > p.mx ? b : p.mx;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { shu[wave * 4] = p.nn; shu[wave * 4 + 1] = p.nan; shu[wave * 4 + 2] = p.mn; shu[wave * 4 + 3] = p.mx; }
    p.sum = ds_block_sum(p.sum, shd);                    // (its barriers order shu too)
    if (threadIdx.x == 0)
        for (int w = 1; w < DS_THREADS / 64; w++) {
            p.nn += shu[w * 4]; p.nan += shu[w * 4 + 1];
            p.mn = shu[w * 4 + 2] < p.mn ? shu[w * 4 + 2] : p.mn;
            p.mx = shu[w * 4 + 3] > p.mx ? shu[w * 4 + 3] : p.mx;
        }
    return p;
}

// ---- 1. moments -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DS_THREADS) void ds_moments_kernel(DsCol c, DsPart *part) {
    __shared__ double shd[DS_THREADS / 64];
    __shared__ uint64_t shu[DS_THREADS / 64 * 4];
    DsPart p{-0.0, 0, 0, ~0ull, 0};                      // Rust's Sum for f64 starts at -0.0
    ds_stream(c, [&](uint64_t b, bool ok) {
        if (!ok) return;
        p.nn++;
        p.sum += ds_value(b, c.i64);
        if (ds_is_nan(b, c.i64)) { p.nan++; return; }
        const uint64_t e = ds_code(b, c.i64);
        p.mn = e < p.mn ? e : p.mn;
        p.mx = e > p.mx ? e : p.mx;
    });
    p = ds_block_part(p, shd, shu);
    if (threadIdx.x == 0) part[blockIdx.x] = p;
}

// percentile()'s ranks (descriptive.rs:182-197): sorted[lo] and sorted[hi] of n values, w = index - lower_index
__device__ __forceinline__ void ds_index(double pc, uint64_t n, uint64_t &lo, uint64_t &hi, double &w) {
    w = 0.0;
    if (pc == 0.0) lo = hi = 0;                          // :182-187: the ends
    else if (pc == 100.0) lo = hi = n - 1;
    else {
        const double index = (pc / 100.0) * (double)(n - 1);          // :190
        lo = (uint64_t)floor(index);
        hi = (uint64_t)ceil(index);
        w = index - (double)lo;                          // :197
    }
    lo = lo < n ? lo : n - 1;                            // (p in [0, 100] keeps both below n; a guard, not a path)
    hi = hi < n ? hi : n - 1;
}

// ---- 2. ranks -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DS_THREADS) void ds_ranks_kernel(const DsPart *part, int n_part, DsReq req, DsState *st) {
    __shared__ double shd[DS_THREADS / 64];
    __shared__ uint64_t shu[DS_THREADS / 64 * 4];
    DsPart p{-0.0, 0, 0, ~0ull, 0};
    for (int i = threadIdx.x; i < n_part; i += DS_THREADS) {
        const DsPart q = part[i];
        p.sum += q.sum; p.nn += q.nn; p.nan += q.nan;
        p.mn = q.mn < p.mn ? q.mn : p.mn;
        p.mx = q.mx > p.mx ? q.mx : p.mx;
    }
    p = ds_block_part(p, shd, shu);
    if (threadIdx.x != 0) return;
    const uint64_t n = p.nn, n_num = p.nn - p.nan;
    st->nn = n; st->nan = p.nan; st->mn = p.mn; st->mx = p.mx;
    st->sum = p.sum;
    st->mean = p.sum / (double)n;                        // descriptive.rs:102
    st->ssq = 0.0;
    st->vary = 0;
    uint64_t lo[DS_MAX_P], hi[DS_MAX_P], tgt[DS_MAX_SLOTS];
    const int n_p = n ? req.n_p : 0;
    int n_t = 0;
    for (int j = 0; j < n_p; j++) {
        double w;
        ds_index(req.p[j], n, lo[j], hi[j], w);
        st->p_w[j] = w;
        tgt[n_t++] = lo[j];
        tgt[n_t++] = hi[j];
    }
    uint64_t rk[DS_MAX_SLOTS];
    const int n_r = n_num ? min(req.rank_n, DS_MAX_SLOTS - n_t) : 0;
    for (int j = 0; j < n_r; j++) {                      // functions.rs:2394-2395; never decreasing in i
        const uint64_t idx = (uint64_t)((double)n_num * (double)(req.rank_i0 + j) / (double)req.rank_q);
        tgt[n_t++] = rk[j] = idx < n_num - 1 ? idx : n_num - 1;
    }
    uint64_t olo[DS_MAX_OS], ohi[DS_MAX_OS];
    const int n_o = min(req.n_os, DS_MAX_OS);
    for (int j = 0; j < n_o; j++) {                      // the reference's four index rules over its sorted `valid` (m = n_num cells)
        const uint64_t m = n_num;
        const double a = req.os_arg[j];
        const uint64_t none = ~0ull;
        olo[j] = ohi[j] = none;
        st->o_t[j] = 0;
        if (!m) continue;
        switch (req.os_op[j]) {
        case PANDRS_HIP_OS_AT_FRAC_N: {                  // aggregations.rs:87-89, :152-153; `as usize` saturates at 0; get() past the end: NaN
            const uint64_t r = a > 0.0 ? (uint64_t)fmin((double)m * a, 1.8e19) : 0;
            if (r < m) olo[j] = ohi[j] = r;
            break;
        }
        case PANDRS_HIP_OS_AT_FRAC_N1: {                 // :198
            const uint64_t r = a > 0.0 ? (uint64_t)fmin((double)(m - 1) * a, 1.8e19) : 0;
            if (r < m) olo[j] = ohi[j] = r;
            break;
        }
        case PANDRS_HIP_OS_MEDIAN:                       // functions.rs:1604-1609
            ohi[j] = m / 2;
            olo[j] = m % 2 == 0 ? m / 2 - 1 : m / 2;
            break;
        case PANDRS_HIP_OS_TRIMMED_MEAN: {               // aggregations.rs:217-218; an empty slice is NaN (:220-222)
            const uint64_t t = a > 0.0 ? (uint64_t)fmin((double)m * a, 1.8e19) : 0;
            st->o_t[j] = t;
            if (t < m - t) { olo[j] = t; ohi[j] = m - 1 - t; }
            break;
        }
        default: break;                                  // -1: answered by the host
        }
        if (olo[j] != none) { tgt[n_t++] = olo[j]; tgt[n_t++] = ohi[j]; }
    }
    for (int a = 1; a < n_t; a++) {                      // ascending, then distinct
        const uint64_t x = tgt[a];
        int b = a - 1;
        while (b >= 0 && tgt[b] > x) { tgt[b + 1] = tgt[b]; b--; }
        tgt[b + 1] = x;
    }
    int n_s = 0;
    bool live = false;
    for (int a = 0; a < n_t; a++) {
        if (n_s && st->s_rank[n_s - 1] == tgt[a]) continue;
        st->s_rank[n_s] = tgt[a];
        st->s_group[n_s] = tgt[a] < n_num ? 0 : -1;
        live = live || tgt[a] < n_num;
        n_s++;
    }
    for (int j = 0; j < n_p; j++)
        for (int s = 0; s < n_s; s++) {
            if (st->s_rank[s] == lo[j]) st->p_lo[j] = s;
            if (st->s_rank[s] == hi[j]) st->p_hi[j] = s;
        }
    for (int j = 0; j < n_r; j++)
        for (int s = 0; s < n_s; s++)
            if (st->s_rank[s] == rk[j]) st->r_slot[j] = s;
    for (int j = 0; j < n_o; j++) {
        st->o_lo[j] = st->o_hi[j] = -1;
        for (int s = 0; s < n_s && olo[j] != ~0ull; s++) {
            if (st->s_rank[s] == olo[j]) st->o_lo[j] = s;
            if (st->s_rank[s] == ohi[j]) st->o_hi[j] = s;
        }
    }
    const uint64_t span = n_num ? p.mx - p.mn : 0;
    const int width = span ? 64 - __clzll((long long)span) : 0;
    st->n_slots = n_s;
    st->n_groups = live ? 1 : 0;
    st->n_pass = live ? (width + DS_DIGIT - 1) / DS_DIGIT : 0;
    st->g_prefix[0] = 0;
}

// ---- 3. selection -----------------------------------------------------------------------------------------------------------
// a digit below the first in which no row has a bit set: every row's digit is 0, so no stream is needed
__device__ __forceinline__ bool ds_digit_is_zero(const DsState *st, int pass) {
    return pass > 0 && pass < st->n_pass && ((st->vary >> (DS_DIGIT * (st->n_pass - 1 - pass))) & (DS_BINS - 1)) == 0;
}

// lanes holding the same (group, digit) as the first pending lane add their number in one LDS atomic
__device__ __forceinline__ void ds_count(uint32_t *h, bool m, uint32_t key) {
    uint64_t todo = __ballot(m);
    const uint32_t lane = threadIdx.x & 63;
    for (int round = 0; todo && round < DS_PEEL; round++) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint32_t k0 = __shfl(key, leader, 64);
        const uint64_t same = __ballot(m && key == k0) & todo;
        if (lane == (uint32_t)leader) atomicAdd(&h[k0], (uint32_t)__popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1) atomicAdd(&h[key], 1u);
}

__global__ __launch_bounds__(DS_THREADS) void ds_select_kernel(DsCol c, const DsState *st, int pass, uint32_t *hist, double *ssq_part,
                                                               unsigned long long *vary) {
    __shared__ uint32_t h[DS_MAX_SLOTS * DS_BINS];
    __shared__ uint64_t pre[DS_MAX_SLOTS];
    __shared__ double shd[DS_THREADS / 64];
    const int n_pass = st->n_pass, G = min(st->n_groups, DS_MAX_SLOTS);
    const bool sel = pass < n_pass && G > 0 && !ds_digit_is_zero(st, pass), do_ssq = pass == 0 && st->nn > 0;
    if (!sel && !do_ssq) return;
    const int shift = sel ? DS_DIGIT * (n_pass - 1 - pass) : 0, hs = shift + DS_DIGIT;
    if (sel) {
        for (int i = threadIdx.x; i < G * DS_BINS; i += DS_THREADS) h[i] = 0;
        if ((int)threadIdx.x < G) pre[threadIdx.x] = st->g_prefix[threadIdx.x];
    }
    __syncthreads();
    const double mean = st->mean;
    const uint64_t mn = st->mn;
    double acc = 0.0;
    uint64_t d_or = 0;
    ds_stream(c, [&](uint64_t b, bool ok) {
        bool m = false;
        uint32_t key = 0;
        if (ok) {
            if (do_ssq) {
                const double d = ds_value(b, c.i64) - mean;        // descriptive.rs:107
                acc += d * d;
            }
            if (sel && !ds_is_nan(b, c.i64)) {
                const uint64_t d = ds_code(b, c.i64) - mn;
                d_or |= d;
                const uint64_t p = hs >= 64 ? 0ull : d >> hs;
                const uint32_t dg = (uint32_t)(d >> shift) & (DS_BINS - 1);
                for (int g = 0; g < G; g++)
                    if (pre[g] == p) { m = true; key = (uint32_t)g * DS_BINS + dg; }
            }
        }
        if (sel) ds_count(h, m, key);
    });
    __syncthreads();
    if (sel)
        for (int i = threadIdx.x; i < G * DS_BINS; i += DS_THREADS)
            if (h[i]) atomicAdd(&hist[i], h[i]);
    if (sel && pass == 0) {                              // which lower digits vary at all
        for (int o = 32; o >= 1; o >>= 1) d_or |= __shfl_down(d_or, o, 64);
        if ((threadIdx.x & 63) == 0 && d_or) atomicOr(vary, (unsigned long long)d_or);
    }
    if (do_ssq) {
        acc = ds_block_sum(acc, shd);
        if (threadIdx.x == 0) ssq_part[blockIdx.x] = acc;
    }
}

__global__ __launch_bounds__(DS_THREADS) void ds_pick_kernel(DsState *st, int pass, uint32_t *hist, const double *ssq_part, int n_part) {
    __shared__ double shd[DS_THREADS / 64];
    __shared__ uint32_t wave_tot[17];
    __shared__ uint32_t new_digit[DS_MAX_SLOTS];
    __shared__ uint64_t new_rank[DS_MAX_SLOTS];
    const int t = threadIdx.x;
    if (pass == 0 && st->nn > 0) {
        double a = 0.0;
        for (int i = t; i < n_part; i += DS_THREADS) a += ssq_part[i];
        a = ds_block_sum(a, shd);
        if (t == 0) st->ssq = a;
    }
    const int G = min(st->n_groups, DS_MAX_SLOTS), n_s = min(st->n_slots, DS_MAX_SLOTS);
    if (pass >= st->n_pass || G <= 0) return;
    if (ds_digit_is_zero(st, pass)) {                    // the chosen digit is 0 for every rank; the ranks stay
        if (t < G) st->g_prefix[t] <<= DS_DIGIT;
        return;
    }
    if (t < DS_MAX_SLOTS) { new_digit[t] = 0; new_rank[t] = t < n_s ? st->s_rank[t] : 0; }
    __syncthreads();
    for (int g = 0; g < G; g++) {
        const uint32_t v = hist[g * DS_BINS + t];
        hist[g * DS_BINS + t] = 0;                       // armed for the next pass
        const uint32_t ex = block_exclusive_scan<DS_THREADS>(v, wave_tot, nullptr);
        for (int s = 0; s < n_s; s++) {
            if (st->s_group[s] != g) continue;
            const uint64_t r = st->s_rank[s];
            if (v && r >= ex && r < (uint64_t)ex + v) { new_digit[s] = (uint32_t)t; new_rank[s] = r - ex; }
        }
    }
    __syncthreads();
    if (t != 0) return;
    // slots are ascending in rank, so ascending in (group, digit): equal neighbours share the new group
    uint64_t np[DS_MAX_SLOTS];
    int ng = 0, prev_g = -1;
    uint32_t prev_d = 0;
    for (int s = 0; s < n_s; s++) {
        const int g = st->s_group[s];
        if (g < 0 || g >= G) continue;
        const uint32_t d = new_digit[s];
        if (g != prev_g || d != prev_d) {
            np[ng++] = (st->g_prefix[g] << DS_DIGIT) | d;
            prev_g = g;
            prev_d = d;
        }
        st->s_group[s] = ng - 1;
        st->s_rank[s] = new_rank[s];
    }
    for (int g = 0; g < ng; g++) st->g_prefix[g] = np[g];
    st->n_groups = ng;
}

// ---- 4. finish --------------------------------------------------------------------------------------------------------------
// out: [0] count (int64), [1 .. 1 + DS_MAX_P) the percentiles, then pandrs_hip_describe_stats
__global__ void ds_finish_kernel(const DsState *st, DsReq req, int i64, int describe, double *out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint64_t n = st->nn, n_num = st->nn - st->nan;
    reinterpret_cast<int64_t *>(out)[0] = (int64_t)n;
    double q[DS_MAX_P];
    for (int j = 0; j < req.n_p; j++) {
        q[j] = NAN;
        if (!n) continue;
        const int sl = st->p_lo[j], sh = st->p_hi[j];
        const double a = st->s_group[sl] < 0 ? (double)NAN : ds_decode(st->mn + st->g_prefix[st->s_group[sl]], i64);
        if (sl == sh) { q[j] = a; continue; }            // descriptive.rs:194-195
        const double b = st->s_group[sh] < 0 ? (double)NAN : ds_decode(st->mn + st->g_prefix[st->s_group[sh]], i64);
        const double w = st->p_w[j];
        q[j] = a * (1.0 - w) + b * w;                    // :198
    }
    for (int j = 0; j < req.n_p; j++) out[1 + j] = q[j];
    if (!describe) return;
    pandrs_hip_describe_stats *ds = reinterpret_cast<pandrs_hip_describe_stats *>(out + 1 + DS_MAX_P);
    ds->count = (int64_t)n;
    if (!n) {
        ds->mean = ds->std = ds->min = ds->q1 = ds->median = ds->q3 = ds->max = NAN;
        return;
    }
    ds->mean = st->mean;
    ds->std = sqrt(st->ssq / (double)(n - 1));           // :107-108; count 1: 0.0 / 0.0
    ds->min = n_num ? ds_decode(st->mn, i64) : (double)NAN;           // sorted[0]; NaN cells order last
    ds->q1 = q[0];
    ds->median = q[1];
    ds->q3 = q[2];
    ds->max = st->nan ? (double)NAN : ds_decode(st->mx, i64);         // sorted[count - 1]
}

// ranks by number.  out: [0] m, the cells that are neither null nor NaN (int64), [1] their min, [2] their max (NaN without
// one), [3 .. 3 + rank_n) the elements at the requested ranks
constexpr int DS_RANK_OUT = 3 + DS_MAX_SLOTS;
__global__ void ds_finish_ranks_kernel(const DsState *st, DsReq req, int i64, double *out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint64_t n_num = st->nn - st->nan;
    reinterpret_cast<int64_t *>(out)[0] = (int64_t)n_num;
    out[1] = n_num ? ds_decode(st->mn, i64) : (double)NAN;
    out[2] = n_num ? ds_decode(st->mx, i64) : (double)NAN;
    for (int j = 0; j < req.rank_n && j < DS_MAX_SLOTS; j++)
        out[3 + j] = n_num ? ds_decode(st->mn + st->g_prefix[st->s_group[st->r_slot[j]]], i64) : (double)NAN;
}

// ---- host side --------------------------------------------------------------------------------------------------------------
// the workspace does not grow with n_rows: per-workgroup partials, the digit counts, the slots, the results
struct DsWork {
    int grid;
    DsPart *part;
    double *ssq_part;
    uint32_t *hist;
    DsState *st;
    double *d_out;
};
constexpr size_t DS_HIST_N = (size_t)DS_MAX_SLOTS * DS_BINS;
constexpr size_t DS_DESCRIBE_OUT = 1 + DS_MAX_P + sizeof(pandrs_hip_describe_stats) / 8;
constexpr size_t DS_OUT_DOUBLES = DS_DESCRIBE_OUT > (size_t)DS_RANK_OUT ? DS_DESCRIBE_OUT : (size_t)DS_RANK_OUT;

static int32_t ds_work(pandrs_hip_ctx *c, int64_t n, const char *who, DsWork &w, size_t extra_per_workgroup = 0) {
    const int64_t tiles = (n + DS_TILE - 1) / DS_TILE;
    w.grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)c->n_cu * DS_BLOCKS_PER_CU, tiles));
    ST_TRY(c->temp.ensure(Arena::padded((size_t)w.grid * sizeof(DsPart)) + Arena::padded((size_t)w.grid * 8) + Arena::padded(DS_HIST_N * 4) +
                          Arena::padded(sizeof(DsState)) + Arena::padded(DS_OUT_DOUBLES * 8) + Arena::padded((size_t)w.grid * extra_per_workgroup) + 4096,
                          c->stream));
    w.part = c->temp.take<DsPart>((size_t)w.grid);
    w.ssq_part = c->temp.take<double>((size_t)w.grid);
    w.hist = c->temp.take<uint32_t>(DS_HIST_N);
    w.st = c->temp.take<DsState>(1);
    w.d_out = c->temp.take<double>(DS_OUT_DOUBLES);
    if (!w.part || !w.ssq_part || !w.hist || !w.st || !w.d_out) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (%s)", who);
    return 0;
}

// moments and ranks, then (select) the eight digit passes; the caller enqueues its finish kernel behind them
static int32_t ds_enqueue(pandrs_hip_ctx *c, const DsCol &dc, const DsReq &req, const DsWork &w, bool select) {
    HIP_TRY(hipMemsetAsync(w.hist, 0, DS_HIST_N * 4, c->stream));
    hipLaunchKernelGGL(ds_moments_kernel, dim3(w.grid), dim3(DS_THREADS), 0, c->stream, dc, w.part);
    hipLaunchKernelGGL(ds_ranks_kernel, dim3(1), dim3(DS_THREADS), 0, c->stream, (const DsPart *)w.part, w.grid, req, w.st);
    HIP_TRY(hipGetLastError());
    for (int pass = 0; select && pass < DS_MAX_PASSES; pass++) {
        hipLaunchKernelGGL(ds_select_kernel, dim3(w.grid), dim3(DS_THREADS), 0, c->stream, dc, (const DsState *)w.st, pass, w.hist, w.ssq_part,
                           reinterpret_cast<unsigned long long *>(&w.st->vary));
        hipLaunchKernelGGL(ds_pick_kernel, dim3(1), dim3(DS_THREADS), 0, c->stream, w.st, pass, w.hist, (const double *)w.ssq_part, w.grid);
    }
    return 0;
}

int32_t describe_entry(pandrs_hip_ctx *c, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows, const double *percentiles,
                       int32_t n_percentiles, double *out_q, int64_t *out_count, pandrs_hip_describe_stats *out_stats) {
    const char *who = out_stats ? "describe" : "quantiles";
    if (!c || !col || n_rows < 0 || (n_rows > 0 && !col->data) || (!out_stats && (!percentiles || !out_q || !out_count)))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "%s: bad arguments", who);
    ST_TRY(check_mem_space(who, mem_space));
    if (col->dtype != PANDRS_HIP_I64 && col->dtype != PANDRS_HIP_F64)
        return fail(PANDRS_HIP_ERR_TYPE_MISMATCH, "%s: the column has dtype %d, expected I64 or F64", who, col->dtype);
    DsReq req{};
    if (out_stats) {
        req.n_p = 3;
        req.p[0] = 25.0; req.p[1] = 50.0; req.p[2] = 75.0;            // descriptive.rs:103, :114-115
    } else {
        if (n_percentiles < 1 || n_percentiles > DS_MAX_P)
            return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "quantiles: %d percentiles; one call takes 1 to %d", n_percentiles, DS_MAX_P);
        req.n_p = n_percentiles;
        for (int j = 0; j < n_percentiles; j++) {
            if (!(percentiles[j] >= 0.0 && percentiles[j] <= 100.0))  // descriptive.rs:176-180; NaN fails both comparisons
                return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "quantiles: percentile %d is %g; it must be between 0 and 100", j, percentiles[j]);
            req.p[j] = percentiles[j];
        }
    }
    if (n_rows >= (int64_t(1) << 32))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "%s: %lld rows; one call takes fewer than 2^32", who, (long long)n_rows);
    std::lock_guard<std::mutex> lock(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    timings_begin(c);
    const int64_t n = n_rows;
    const size_t out_doubles = DS_DESCRIBE_OUT;
    double *h_out = static_cast<double *>(c->pinned);
    if (n == 0) {                                           // no cell at all: count 0, NaN results
        reinterpret_cast<int64_t *>(h_out)[0] = 0;
        for (size_t i = 1; i < out_doubles; i++) h_out[i] = NAN;
        reinterpret_cast<int64_t *>(h_out + 1 + DS_MAX_P)[0] = 0;
        ST_TRY(timings_end(c));
    } else {
        DsWork w{};
        ST_TRY(ds_work(c, n, who, w));
        ColView cv{col->data, col->null_mask};
        Stager stg{c, mem_space};
        if (const size_t need = stg.col_size(*col, n)) {
            PhaseTimer pt(c, PANDRS_HIP_PHASE_STAGE_IN);
            ST_TRY(stg.reserve(need));
            cv = stg.col(*col, n);
            if (stg.status) return stg.status;
        }
        if (reinterpret_cast<uintptr_t>(cv.data) & 7) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "%s: the column must be 8-byte aligned", who);
        const DsCol dc{static_cast<const uint64_t *>(cv.data), cv.mask, n, col->dtype == PANDRS_HIP_I64 ? 1 : 0};
        {
            PhaseTimer pt(c, PANDRS_HIP_PHASE_OTHER);
            ST_TRY(ds_enqueue(c, dc, req, w, true));
            hipLaunchKernelGGL(ds_finish_kernel, dim3(1), dim3(64), 0, c->stream, (const DsState *)w.st, req, dc.i64, out_stats ? 1 : 0, w.d_out);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(h_out, w.d_out, out_doubles * 8, hipMemcpyDeviceToHost, c->stream));
        c->timings.algorithmic_bytes = (int64_t)n * 8 + (col->null_mask ? (n + 7) / 8 : 0);      // the column (+ mask), once
        ST_TRY(timings_end(c));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (out_stats) std::memcpy(out_stats, h_out + 1 + DS_MAX_P, sizeof *out_stats);
    else {
        *out_count = reinterpret_cast<const int64_t *>(h_out)[0];
        for (int j = 0; j < req.n_p; j++) out_q[j] = h_out[1 + j];
    }
    return 0;
}

// The reference's edge list (functions.rs:2349-2351, :2392-2397).  CUT: min and max from the moments pass, the edges built here.
// QCUT(k): the k + 1 elements at the ranks above, DS_MAX_SLOTS per selection, so k + 1 > DS_MAX_SLOTS runs
// ceil((k + 1) / DS_MAX_SLOTS) selections over the column, each with its own moments pass: correct, not fast.
int32_t bin_edges_entry(pandrs_hip_ctx *c, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows, int32_t kind, int32_t k,
                        double *out_edges, int64_t *out_valid) {
    if (!c || !col || n_rows < 0 || (n_rows > 0 && !col->data) || !out_edges || !out_valid)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "bin_edges: bad arguments");
    ST_TRY(check_mem_space("bin_edges", mem_space));
    if (kind != PANDRS_HIP_BIN_CUT && kind != PANDRS_HIP_BIN_QCUT)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "bin_edges: kind %d is not a pandrs_hip_bin_kind", kind);
    if (col->dtype != PANDRS_HIP_I64 && col->dtype != PANDRS_HIP_F64)
        return fail(PANDRS_HIP_ERR_TYPE_MISMATCH, "bin_edges: the column has dtype %d, expected I64 or F64", col->dtype);
    if (k < 1 || k > PANDRS_HIP_BIN_MAX_BINS)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "bin_edges: k = %d; one call takes 1 to %d", k, PANDRS_HIP_BIN_MAX_BINS);
    if (n_rows >= (int64_t(1) << 32))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "bin_edges: %lld rows; one call takes fewer than 2^32", (long long)n_rows);
    *out_valid = 0;
    for (int32_t i = 0; i <= k; i++) out_edges[i] = NAN;
    if (n_rows == 0) return 0;
    std::lock_guard<std::mutex> lock(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    timings_begin(c);
    const int64_t n = n_rows;
    DsWork w{};
    ST_TRY(ds_work(c, n, "bin_edges", w));
    ColView cv{col->data, col->null_mask};
    Stager stg{c, mem_space};
    if (const size_t need = stg.col_size(*col, n)) {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_STAGE_IN);
        ST_TRY(stg.reserve(need));
        cv = stg.col(*col, n);
        if (stg.status) return stg.status;
    }
    if (reinterpret_cast<uintptr_t>(cv.data) & 7) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "bin_edges: the column must be 8-byte aligned");
    const DsCol dc{static_cast<const uint64_t *>(cv.data), cv.mask, n, col->dtype == PANDRS_HIP_I64 ? 1 : 0};
    // one block of DS_RANK_OUT doubles per selection in the pinned block; the copies are ordered by the stream
    const int n_sel = kind == PANDRS_HIP_BIN_QCUT ? (k + 1 + DS_MAX_SLOTS - 1) / DS_MAX_SLOTS : 1;
    static_assert(((size_t)PANDRS_HIP_BIN_MAX_BINS + 1 + DS_MAX_SLOTS - 1) / DS_MAX_SLOTS * DS_RANK_OUT * 8 <= (1 << 16),
                  "the selections of a call fit the context's pinned block");
    double *h_out = static_cast<double *>(c->pinned);
    {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_OTHER);
        for (int s = 0; s < n_sel; s++) {
            DsReq req{};
            if (kind == PANDRS_HIP_BIN_QCUT) {
                req.rank_q = k;
                req.rank_i0 = s * DS_MAX_SLOTS;
                req.rank_n = std::min(DS_MAX_SLOTS, k + 1 - req.rank_i0);
            }
            ST_TRY(ds_enqueue(c, dc, req, w, kind == PANDRS_HIP_BIN_QCUT));
            hipLaunchKernelGGL(ds_finish_ranks_kernel, dim3(1), dim3(64), 0, c->stream, (const DsState *)w.st, req, dc.i64, w.d_out);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(h_out + (size_t)s * DS_RANK_OUT, w.d_out, (size_t)DS_RANK_OUT * 8, hipMemcpyDeviceToHost, c->stream));
        }
    }
    c->timings.n_partitions = n_sel;
    c->timings.algorithmic_bytes = (int64_t)n * 8 + (col->null_mask ? (n + 7) / 8 : 0);          // the column (+ mask), once
    ST_TRY(timings_end(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int64_t m = reinterpret_cast<const int64_t *>(h_out)[0];
    *out_valid = m;
    if (m == 0) return 0;                                // (the edges stay NaN)
    if (kind == PANDRS_HIP_BIN_QCUT) {
        for (int32_t i = 0; i <= k; i++) out_edges[i] = h_out[(size_t)(i / DS_MAX_SLOTS) * DS_RANK_OUT + 3 + i % DS_MAX_SLOTS];
        return 0;
    }
    // functions.rs:2349-2351, every operation rounded on its own: this file compiles with fp contract(off), so i * w + min is a
    // multiplication and an addition, never a fused multiply-add
    const double mn = h_out[1], mx = h_out[2];
    const double width = (mx - mn) / (double)k;
    for (int32_t i = 0; i <= k; i++) out_edges[i] = mn + (double)i * width;
    out_edges[k] = mx + 0.001;
    return 0;
}

// ---- 6. order statistics by the reference's index rules (pandrs_hip_order_stats) ---------------------------------------------------
// Steps 1 to 3 with the ranks of ds_ranks_kernel's four rules, counted over the cells that are neither null nor NaN.  TRIMMED_MEAN
// then takes one band stream: the sum of the cells whose code lies strictly between the two selected codes, and how many cells lie
// below, on the lower code, on the upper code and above; the finish adds the cut values as often as the sorted slice holds them.
struct DsBand {
    double sum;
    uint64_t below, eq_lo, eq_hi, above;
};

__device__ __forceinline__ uint64_t ds_slot_code(const DsState *st, int slot) { return st->mn + st->g_prefix[st->s_group[slot]]; }

__global__ __launch_bounds__(DS_THREADS) void ds_band_kernel(DsCol c, const DsState *st, int op, DsBand *part) {
    __shared__ double shd[DS_THREADS / 64];
    __shared__ uint64_t shu[DS_THREADS / 64];
    const int sl = st->o_lo[op], sh = st->o_hi[op];
    if (sl < 0 || sh < 0) return;                        // (uniform) an empty slice or no cell: NaN without a stream
    const uint64_t lo = ds_slot_code(st, sl), hi = ds_slot_code(st, sh);
    DsBand b{-0.0, 0, 0, 0, 0};
    ds_stream(c, [&](uint64_t bits, bool ok) {
        if (!ok || ds_is_nan(bits, c.i64)) return;
        const uint64_t e = ds_code(bits, c.i64);
        if (e < lo) b.below++;
        else if (e == lo) b.eq_lo++;
        else if (e < hi) b.sum += ds_value(bits, c.i64);
        else if (e == hi) b.eq_hi++;
        else b.above++;
    });
    b.sum = ds_block_sum(b.sum, shd);
    b.below = ds_block_count(b.below, shu);
    b.eq_lo = ds_block_count(b.eq_lo, shu);
    b.eq_hi = ds_block_count(b.eq_hi, shu);
    b.above = ds_block_count(b.above, shu);
    if (threadIdx.x == 0) part[(size_t)op * gridDim.x + blockIdx.x] = b;
}

// out: [0] m, the cells that are neither null nor NaN (int64), [1 .. 1 + n_os) the results
__global__ __launch_bounds__(DS_THREADS) void ds_finish_os_kernel(const DsState *st, DsReq req, int i64, const DsBand *part, int n_part, double *out) {
    __shared__ double shd[DS_THREADS / 64];
    __shared__ uint64_t shu[DS_THREADS / 64];
    const uint64_t m = st->nn - st->nan;
    if (threadIdx.x == 0) reinterpret_cast<int64_t *>(out)[0] = (int64_t)m;
    for (int j = 0; j < req.n_os && j < DS_MAX_OS; j++) {
        const int sl = st->o_lo[j], sh = st->o_hi[j];
        if (sl < 0 || sh < 0) {                          // (uniform)
            if (threadIdx.x == 0) out[1 + j] = NAN;
            continue;
        }
        const double v_lo = ds_decode(ds_slot_code(st, sl), i64), v_hi = ds_decode(ds_slot_code(st, sh), i64);
        if (req.os_op[j] != PANDRS_HIP_OS_TRIMMED_MEAN) {
            if (threadIdx.x == 0) out[1 + j] = req.os_op[j] == PANDRS_HIP_OS_MEDIAN && sl != sh ? (v_lo + v_hi) / 2.0 : v_lo;
            continue;
        }
        DsBand b{-0.0, 0, 0, 0, 0};
        for (int i = threadIdx.x; i < n_part; i += DS_THREADS) {
            const DsBand q = part[(size_t)j * n_part + i];
            b.sum += q.sum; b.below += q.below; b.eq_lo += q.eq_lo; b.eq_hi += q.eq_hi; b.above += q.above;
        }
        b.sum = ds_block_sum(b.sum, shd);
        b.below = ds_block_count(b.below, shu);
        b.eq_lo = ds_block_count(b.eq_lo, shu);
        b.eq_hi = ds_block_count(b.eq_hi, shu);
        b.above = ds_block_count(b.above, shu);
        if (threadIdx.x != 0) continue;
        const uint64_t t = st->o_t[j], kept = m - 2 * t;
        double num;
        if (ds_slot_code(st, sl) == ds_slot_code(st, sh)) num = (double)kept * v_lo;       // both cuts select one code: the slice holds nothing else
        else num = b.sum + (double)(b.below + b.eq_lo - t) * v_lo + (double)(b.eq_hi + b.above - t) * v_hi;
        out[1 + j] = num / (double)kept;                 // aggregations.rs:224
    }
}

int32_t order_stats_entry(pandrs_hip_ctx *c, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows, const int32_t *ops,
                          const double *args, int32_t n_ops, double *out, int64_t *out_count) {
    if (!c || !col || n_rows < 0 || (n_rows > 0 && !col->data) || !ops || !args || !out || !out_count)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "order_stats: bad arguments");
    ST_TRY(check_mem_space("order_stats", mem_space));
    if (col->dtype != PANDRS_HIP_I64 && col->dtype != PANDRS_HIP_F64)
        return fail(PANDRS_HIP_ERR_TYPE_MISMATCH, "order_stats: the column has dtype %d, expected I64 or F64", col->dtype);
    if (n_ops < 1 || n_ops > DS_MAX_OS)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "order_stats: %d ops; one call takes 1 to %d (two ranks each, %d slots)", n_ops, DS_MAX_OS,
                    DS_MAX_SLOTS);
    DsReq req{};
    req.n_os = n_ops;
    bool band = false;
    for (int j = 0; j < n_ops; j++) {
        const double a = args[j];
        if (ops[j] < PANDRS_HIP_OS_AT_FRAC_N || ops[j] > PANDRS_HIP_OS_TRIMMED_MEAN)
            return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "order_stats: op %d is %d, not a pandrs_hip_order_stat", j, ops[j]);
        if (a != a && ops[j] != PANDRS_HIP_OS_MEDIAN)
            return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "order_stats: the argument of op %d is NaN", j);
        req.os_op[j] = ops[j];
        req.os_arg[j] = a;
        // the reference's early returns, decided before any launch: percentile_value's q (aggregations.rs:185), trimmed_mean's fraction (:204)
        if ((ops[j] == PANDRS_HIP_OS_AT_FRAC_N1 && (a < 0.0 || a > 1.0)) || (ops[j] == PANDRS_HIP_OS_TRIMMED_MEAN && (a < 0.0 || a >= 0.5)))
            req.os_op[j] = -1;
        band = band || req.os_op[j] == PANDRS_HIP_OS_TRIMMED_MEAN;
    }
    if (n_rows >= (int64_t(1) << 32))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "order_stats: %lld rows; one call takes fewer than 2^32", (long long)n_rows);
    *out_count = 0;
    for (int j = 0; j < n_ops; j++) out[j] = NAN;
    if (n_rows == 0) return 0;
    std::lock_guard<std::mutex> lock(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    timings_begin(c);
    const int64_t n = n_rows;
    DsWork w{};
    ST_TRY(ds_work(c, n, "order_stats", w, (size_t)DS_MAX_OS * sizeof(DsBand)));
    DsBand *band_part = c->temp.take<DsBand>((size_t)w.grid * DS_MAX_OS);
    if (!band_part) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (order_stats)");
    ColView cv{col->data, col->null_mask};
    Stager stg{c, mem_space};
    if (const size_t need = stg.col_size(*col, n)) {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_STAGE_IN);
        ST_TRY(stg.reserve(need));
        cv = stg.col(*col, n);
        if (stg.status) return stg.status;
    }
    if (reinterpret_cast<uintptr_t>(cv.data) & 7) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "order_stats: the column must be 8-byte aligned");
    const DsCol dc{static_cast<const uint64_t *>(cv.data), cv.mask, n, col->dtype == PANDRS_HIP_I64 ? 1 : 0};
    double *h_out = static_cast<double *>(c->pinned);
    int n_band = 0;
    {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_OTHER);
        ST_TRY(ds_enqueue(c, dc, req, w, true));
        for (int j = 0; j < n_ops; j++)
            if (req.os_op[j] == PANDRS_HIP_OS_TRIMMED_MEAN) {
                hipLaunchKernelGGL(ds_band_kernel, dim3(w.grid), dim3(DS_THREADS), 0, c->stream, dc, (const DsState *)w.st, j, band_part);
                n_band++;
            }
        hipLaunchKernelGGL(ds_finish_os_kernel, dim3(1), dim3(DS_THREADS), 0, c->stream, (const DsState *)w.st, req, dc.i64, (const DsBand *)band_part,
                           w.grid, w.d_out);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(h_out, w.d_out, (size_t)(1 + DS_MAX_OS) * 8, hipMemcpyDeviceToHost, c->stream));
    c->timings.n_partitions = n_band;                    // the band streams behind the selection
    c->timings.algorithmic_bytes = (int64_t)n * 8 + (col->null_mask ? (n + 7) / 8 : 0);          // the column (+ mask), once
    ST_TRY(timings_end(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out_count = reinterpret_cast<const int64_t *>(h_out)[0];
    for (int j = 0; j < n_ops; j++) out[j] = h_out[1 + j];
    return 0;
}

}  // namespace pandrs
