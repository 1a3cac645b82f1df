// window_quantile.hip — rolling and expanding median / quantile behind Rolling::{median, quantile} and Expanding::{median,
// quantile} (reference src/series/window.rs:298-336, :494-530 over the bounds of :163-203 / :379-400) and
// PandasCompatExt::rolling_median (helpers/window_ops.rs:206-240), gfx950, wave64.  One numeric column (F64 as is, I64
// `as f64`); a window's values are its included cells (non-null; with nan_missing also non-NaN) in the order of the
// reference's stable sort_by(partial_cmp): ascending, -0.0 and +0.0 tied, ties in row order.
//
// A. General path (any window, centred or not, expanding): a wavelet matrix over sort ranks.
//    1. Ranks.  The stable radix sort of sort.hip (sort_order_device) orders numbers ascending with -0.0 == 0.0 tied in row
//       order, then NaN, then nulls: its order restricted to a window's rows is that window's sorted order, and excluded
//       rows rank above every included one.  wq_rank_kernel scatters rank[perm[p]] = p and gathers the original cell
//       sorted_val[p] (not the key: -0.0 survives).
//    2. Levels.  L = the bit length of n-1 (at least 1).  For each bit from the top down: every 4096-row tile counts its one
//       bits (wq_count_kernel: wave ballots), one workgroup scans the tile counts (wq_scan_kernel), and the split
//       (wq_split_kernel) writes the level's words {64 bits, ones before} and moves the ranks stably, zeros first, into the
//       other rank buffer.  Every hand-off between workgroups is a kernel boundary; no workgroup waits on another.  One
//       rank query is one 16-byte load.  The word of position n exists too, so rank(n) needs no special case.
//    3. The included rows (and, without nan_missing, the NaN cells) get a bit vector of the same shape over row order, so a
//       window's len is two look-ups.
//    4. wq_query_kernel: one thread per output descends the L levels with k (both k of an even median share the descent
//       until they part), rebuilds the rank from the branch bits and reads sorted_val[rank].
// B. Direct path (rolling, w <= WQ_DIRECT_MAX): a workgroup stages the order-preserving keys of its WQ_DT outputs' windows
//    in LDS (excluded cells: a sentinel above every number); each thread finds, for its window, the cell whose number of
//    predecessors (smaller key, or equal key and earlier row) is k.  O(w^2) LDS reads, no sort, no workspace.  Lane i
//    reads keys[i + j]: consecutive 8-byte words, no bank conflict.
#include "window.hpp"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace pandrs {

constexpr int WQ_DIRECT_MAX = 44;              // widest window of the direct path (experiments/window_quantile_bench.py)
constexpr int WQ_DT = WN_THREADS;              // direct path: outputs per workgroup, one per thread
constexpr int WQ_TILE = 4096;                  // rows per tile of the level kernels: 4 waves x WQ_WPW words of 64 rows
constexpr int WQ_WPW = 16;
constexpr int WQ_TILE_WORDS = WQ_TILE / 64;
constexpr uint64_t WQ_KEY_NAN = 0xFFFFFFFFFFFFFFFEull;     // direct path: a NaN value that is not missing
constexpr uint64_t WQ_KEY_OUT = 0xFFFFFFFFFFFFFFFFull;     //              an excluded cell; both above +inf's key

struct alignas(16) WqWord {
    uint64_t bits;
    uint32_t ones;             // one bits of the vector before this word
    uint32_t pad;
};

// ---- what k a window of len included cells selects (series/window.rs:302-307, :327-328) ----------------------------------
struct WqStat {
    int median;
    double q;
    __device__ __forceinline__ void ks(int64_t len, int64_t &k1, int64_t &k2) const {       // len >= 1
        if (median) {
            const int64_t mid = len / 2;
            k2 = mid;
            k1 = (len & 1) ? mid : mid - 1;
        } else {
            const int64_t idx = (int64_t)round(q * (double)(len - 1));          // Rust's f64::round: half away from zero
            k1 = k2 = idx < len - 1 ? idx : len - 1;
        }
    }
    __device__ __forceinline__ static double result(double a, double b, bool two) { return two ? (a + b) / 2.0 : a; }
};

// ---- B. the direct path ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t wq_key(double x) {            // x is not NaN
    if (x == 0.0) x = 0.0;                                        // -0.0 ties with +0.0
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    return (b >> 63) ? ~b : b | (1ull << 63);
}

__global__ __launch_bounds__(WN_THREADS) void wq_direct_kernel(WnCol col, WnGeom g, int64_t min_periods, WqStat st, int nan_missing,
                                                                double *out) {
    __shared__ uint64_t keys[WQ_DT + WQ_DIRECT_MAX];
    const int64_t n = g.n, T0 = (int64_t)blockIdx.x * WQ_DT, T1 = std::min<int64_t>(T0 + WQ_DT, n);
    int64_t S, E, tmp;
    g.bounds(T0, S, tmp);
    g.bounds(T1 - 1, tmp, E);                                      // the bounds grow with i: the windows' union is [S, E)
    const int span = (int)std::min<int64_t>(E - S, WQ_DT + WQ_DIRECT_MAX);
    for (int p = threadIdx.x; p < span; p += WN_THREADS) {
        const int64_t r = S + p;
        uint64_t k = WQ_KEY_OUT;
        if (col.valid(r)) {
            const double x = col.x(r);
            k = isnan(x) ? (nan_missing ? WQ_KEY_OUT : WQ_KEY_NAN) : wq_key(x);
        }
        keys[p] = k;
    }
    __syncthreads();
    const int64_t i = T0 + threadIdx.x;
    if (i >= n) return;
    int64_t s, e;
    g.bounds(i, s, e);
    const int a = (int)(s - S), b = std::min((int)(e - S), span);
    int len = 0;
    bool has_nan = false;
    for (int j = a; j < b; j++) {
        const uint64_t k = keys[j];
        len += k != WQ_KEY_OUT;
        has_nan |= k == WQ_KEY_NAN;
    }
    double r = NAN;
    if (len >= min_periods && len > 0 && !has_nan) {
        int64_t k1, k2;
        st.ks(len, k1, k2);
        int c1 = a, c2 = a;
        for (int c = a; c < b; c++) {
            const uint64_t kc = keys[c];
            if (kc == WQ_KEY_OUT) continue;
            int before = 0;                                        // predecessors: an equal key counts only from an earlier row
            for (int j = a; j < c; j++) before += keys[j] <= kc;
            for (int j = c + 1; j < b; j++) before += keys[j] < kc;
            if (before == (int)k1) c1 = c;
            if (before == (int)k2) c2 = c;
        }
        r = WqStat::result(col.x(S + c1), col.x(S + c2), k1 != k2);
    }
    out[i] = r;
}

// ---- A. the general path --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wq_rank_kernel(const int64_t *perm, WnCol col, uint32_t *rank, double *sorted_val) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= col.n) return;
    const int64_t row = perm[p];
    if ((uint64_t)row >= (uint64_t)col.n) return;                 // (cannot happen with a permutation; a guard, not a path)
    rank[row] = (uint32_t)p;
    sorted_val[p] = col.x(row);
}

// the bit of a row, and the value the split moves with it
struct WqRankBit {
    const uint32_t *a;
    int shift;
    __device__ __forceinline__ bool operator()(int64_t r, uint32_t &v) const {
        v = a[r];
        return (v >> shift) & 1u;
    }
};
struct WqInclBit {             // the cell is one of its windows' values
    WnCol col;
    int nan_missing;
    __device__ __forceinline__ bool operator()(int64_t r, uint32_t &) const {
        return col.valid(r) && !(nan_missing && !col.i64 && isnan(col.x(r)));
    }
};
struct WqNanBit {              // a NaN value (not missing): its windows answer NaN
    WnCol col;
    __device__ __forceinline__ bool operator()(int64_t r, uint32_t &) const { return col.valid(r) && !col.i64 && isnan(col.x(r)); }
};

template <class Src>
__global__ __launch_bounds__(WN_THREADS) void wq_count_kernel(Src src, int64_t n, uint32_t *tile_ones) {
    __shared__ uint32_t sh[WN_THREADS / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t w0 = (int64_t)blockIdx.x * WQ_TILE_WORDS + wave * WQ_WPW;
    uint32_t cnt = 0;
    for (int j = 0; j < WQ_WPW; j++) {
        const int64_t r = (w0 + j) * 64 + lane;
        uint32_t v;
        const bool bit = r < n && src(r, v);
        cnt += (uint32_t)__popcll(__ballot(bit));
    }
    if (lane == 0) sh[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) tile_ones[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// one workgroup: carry[t] = the one bits before tile t; *zeros = the vector's zero bits
__global__ __launch_bounds__(WN_THREADS) void wq_scan_kernel(const uint32_t *tile_ones, int64_t n_tiles, int64_t n, uint32_t *carry,
                                                              uint32_t *zeros) {
    __shared__ uint32_t sh[WN_THREADS];
    const int t = threadIdx.x;
    const int64_t per = (n_tiles + WN_THREADS - 1) / WN_THREADS;
    const int64_t a = std::min<int64_t>(n_tiles, (int64_t)t * per), b = std::min<int64_t>(n_tiles, a + per);
    uint32_t v = 0;
    for (int64_t k = a; k < b; k++) v += tile_ones[k];
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < WN_THREADS; o <<= 1) {
        const uint32_t u = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += u;
        __syncthreads();
    }
    uint32_t run = t ? sh[t - 1] : 0;
    for (int64_t k = a; k < b; k++) {
        carry[k] = run;
        run += tile_ones[k];
    }
    if (t == WN_THREADS - 1) *zeros = (uint32_t)((uint64_t)n - sh[WN_THREADS - 1]);
}

// the level's words, and (SCATTER) the stable split of the values: zeros keep their order in [0, Z), ones in [Z, n)
template <class Src, bool SCATTER>
__global__ __launch_bounds__(WN_THREADS) void wq_split_kernel(Src src, int64_t n, int64_t n_words, const uint32_t *carry,
                                                               const uint32_t *zeros, WqWord *words, uint32_t *dst) {
    __shared__ uint32_t sh[WN_THREADS / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t w0 = (int64_t)blockIdx.x * WQ_TILE_WORDS + wave * WQ_WPW;
    uint64_t bits[WQ_WPW];
    uint32_t val[WQ_WPW];
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < WQ_WPW; j++) {
        const int64_t r = (w0 + j) * 64 + lane;
        val[j] = 0;
        const bool bit = r < n && src(r, val[j]);
        bits[j] = __ballot(bit);
        cnt += (uint32_t)__popcll(bits[j]);
    }
    if (lane == 0) sh[wave] = cnt;
    __syncthreads();
    uint32_t run = carry[blockIdx.x];
    for (int k = 0; k < wave; k++) run += sh[k];
    const uint64_t Z = SCATTER ? *zeros : 0;
#pragma unroll
    for (int j = 0; j < WQ_WPW; j++) {
        const int64_t wi = w0 + j, r = wi * 64 + lane;
        if (lane == 0 && wi < n_words) words[wi] = WqWord{bits[j], run, 0u};
        if (SCATTER && r < n) {
            const uint64_t before = run + (uint64_t)__popcll(bits[j] & ((1ull << lane) - 1));
            const uint64_t pos = ((bits[j] >> lane) & 1) ? Z + before : (uint64_t)r - before;
            if (pos < (uint64_t)n) dst[pos] = val[j];             // (always, with consistent counts; a guard, not a path)
        }
        run += (uint32_t)__popcll(bits[j]);
    }
}

struct WqQuery {
    const WqWord *levels;      // [L][n_words]
    const uint32_t *zeros;     // [L]
    const WqWord *incl, *nanv; // row order; nanv == nullptr: no NaN vector (nan_missing, or an I64 column)
    const double *sorted_val;
    WnGeom g;
    int64_t n_words, min_periods;
    int L, expanding;
    WqStat st;
};

__device__ __forceinline__ int64_t wq_rank1(const WqWord *v, int64_t pos) {
    const WqWord w = v[pos >> 6];
    return (int64_t)w.ones + __popcll(w.bits & ((1ull << (pos & 63)) - 1));
}

struct WqNode {
    int64_t s, e, k;
    uint32_t rank;
    // one level down: to the zero side while k is among the node's zeros, else past them to the one side
    __device__ __forceinline__ void step(const WqWord *lv, int64_t Z, int bit) {
        const int64_t os = wq_rank1(lv, s), oe = wq_rank1(lv, e);
        const int64_t c0 = (e - s) - (oe - os);
        if (k < c0) { s -= os; e -= oe; }
        else { k -= c0; s = Z + os; e = Z + oe; rank |= 1u << bit; }
    }
};

__global__ __launch_bounds__(WN_THREADS) void wq_query_kernel(WqQuery Q, double *out) {
    const int64_t i = (int64_t)blockIdx.x * WN_THREADS + threadIdx.x;
    if (i >= Q.g.n) return;
    int64_t s = 0, e = i + 1;
    if (!Q.expanding) Q.g.bounds(i, s, e);
    const int64_t len = wq_rank1(Q.incl, e) - wq_rank1(Q.incl, s);
    double r = NAN;
    if (len >= Q.min_periods && len > 0 && !(Q.nanv && wq_rank1(Q.nanv, e) != wq_rank1(Q.nanv, s))) {
        int64_t k1, k2;
        Q.st.ks(len, k1, k2);
        const bool two = k1 != k2;                                 // an even median: k2 = k1 + 1
        WqNode A{s, e, k1, 0u}, B{s, e, k2, 0u};
        bool parted = false;                                       // the two share one descent until a level separates them
        for (int l = 0; l < Q.L; l++) {
            const WqWord *lv = Q.levels + (size_t)l * Q.n_words;
            const int64_t Z = Q.zeros[l];
            const int bit = Q.L - 1 - l;
            if (two && !parted) {
                const int64_t os = wq_rank1(lv, A.s), oe = wq_rank1(lv, A.e);
                const int64_t c0 = (A.e - A.s) - (oe - os);
                if (A.k + 1 == c0) {                               // k1 is the node's last zero, k2 its first one
                    B = WqNode{Z + os, Z + oe, 0, A.rank | (1u << bit)};
                    parted = true;
                }
                if (A.k < c0) { A.s -= os; A.e -= oe; }
                else { A.k -= c0; A.s = Z + os; A.e = Z + oe; A.rank |= 1u << bit; }
            } else {
                A.step(lv, Z, bit);
                if (parted) B.step(lv, Z, bit);
            }
        }
        r = WqStat::result(Q.sorted_val[A.rank], Q.sorted_val[parted ? B.rank : A.rank], two);
    }
    out[i] = r;
}

// ---- host side ------------------------------------------------------------------------------------------------------------
namespace {

int wq_levels(int64_t n) {
    int L = 1;
    while (L < 32 && ((int64_t)1 << L) < n) L++;                  // the bit length of n - 1, at least 1
    return L;
}

// c->work bytes of the general path on top of the sort's and the permutation (sort_order_device's extra_work)
size_t wq_workspace(int64_t n) {
    const size_t n_words = (size_t)n / 64 + 1, tiles = (n_words + WQ_TILE_WORDS - 1) / WQ_TILE_WORDS;
    return 2 * Arena::padded((size_t)n * 4) + Arena::padded((size_t)n * 8) + Arena::padded(((size_t)wq_levels(n) + 2) * n_words * sizeof(WqWord)) +
           2 * Arena::padded(tiles * 4) + Arena::padded(64 * 4);
}

template <class Src>
int32_t wq_vector(pandrs_hip_ctx *c, const Src &src, int64_t n, int64_t n_words, uint32_t *tile_ones, uint32_t *carry, uint32_t *zeros,
                  WqWord *words, uint32_t *dst) {
    const unsigned tiles = (unsigned)((n_words + WQ_TILE_WORDS - 1) / WQ_TILE_WORDS);
    hipLaunchKernelGGL(wq_count_kernel<Src>, dim3(tiles), dim3(WN_THREADS), 0, c->stream, src, n, tile_ones);
    hipLaunchKernelGGL(wq_scan_kernel, dim3(1), dim3(WN_THREADS), 0, c->stream, (const uint32_t *)tile_ones, (int64_t)tiles, n, carry, zeros);
    if (dst) hipLaunchKernelGGL((wq_split_kernel<Src, true>), dim3(tiles), dim3(WN_THREADS), 0, c->stream, src, n, n_words,
                                (const uint32_t *)carry, (const uint32_t *)zeros, words, dst);
    else hipLaunchKernelGGL((wq_split_kernel<Src, false>), dim3(tiles), dim3(WN_THREADS), 0, c->stream, src, n, n_words,
                            (const uint32_t *)carry, (const uint32_t *)zeros, words, dst);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

int32_t window_quantile_entry(pandrs_hip_ctx *c, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows,
                              const pandrs_hip_window_quantile_spec *spec, int32_t out_mem_space, double *out) {
    if (!c || !col || !spec || n_rows < 0 || (n_rows > 0 && (!col->data || !out)))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "window_quantile: bad arguments");
    ST_TRY(check_mem_space("window_quantile", mem_space, out_mem_space));
    if (col->dtype != PANDRS_HIP_I64 && col->dtype != PANDRS_HIP_F64)
        return fail(PANDRS_HIP_ERR_TYPE_MISMATCH, "window_quantile: the column has dtype %d, expected I64 or F64", col->dtype);
    const pandrs_hip_window_quantile_spec sp = *spec;
    const bool rolling = sp.kind == PANDRS_HIP_WINDOW_KIND_ROLLING;
    if (!rolling && sp.kind != PANDRS_HIP_WINDOW_KIND_EXPANDING)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "window_quantile: kind %d is neither ROLLING nor EXPANDING", sp.kind);
    if ((sp.median != 0 && sp.median != 1) || (sp.nan_missing != 0 && sp.nan_missing != 1))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "window_quantile: median %d, nan_missing %d (each 0 or 1)", sp.median, sp.nan_missing);
    if (rolling && (sp.window < 1 || (sp.center != 0 && sp.center != 1)))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "window_quantile: window_size %lld (must be >= 1), center %d", (long long)sp.window, sp.center);
    if (!rolling && sp.min_periods < 0)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "window_quantile: expanding min_periods %lld < 0", (long long)sp.min_periods);
    if (!sp.median && !(sp.q >= 0.0 && sp.q <= 1.0))              // (a NaN q fails both comparisons)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "window_quantile: Quantile must be between 0 and 1");
    if (n_rows >= (int64_t(1) << 32))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "window_quantile: %lld rows; one call takes fewer than 2^32", (long long)n_rows);
    std::lock_guard<std::mutex> lock(c->mu);
    const int64_t path = c->opt.window_quantile_path;
    const bool fits_direct = rolling && sp.window <= WQ_DIRECT_MAX;
    if (path == 1 && !fits_direct)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "window_quantile: the direct path takes rolling windows of at most %d rows", WQ_DIRECT_MAX);
    const bool direct = fits_direct && path != 2;
    HIP_TRY(hipSetDevice(c->device));
    timings_begin(c);
    if (n_rows == 0) return timings_end(c);
    const int64_t n = n_rows;
    const size_t dbytes = (size_t)n * 8, mbytes = (size_t)(n + 7) / 8;
    const bool has_null = col->null_mask != nullptr;
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
    if (reinterpret_cast<uintptr_t>(cv.data) & 7) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "window_quantile: the column must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_out) & 7) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "window_quantile: the output must be 8-byte aligned");

    const int i64 = col->dtype == PANDRS_HIP_I64 ? 1 : 0;
    const WnCol wc{cv.data, cv.mask, n, (int64_t)mbytes, i64};
    const int64_t w = rolling ? std::min<int64_t>(sp.window, 2 * n + 2) : n;
    const WnGeom g{n, w, w / 2, rolling ? sp.center : 0};
    const int64_t mp = rolling && sp.min_periods < 0 ? sp.window : sp.min_periods;       // series/window.rs:146
    const WqStat st{sp.median, sp.q};
    if (direct) {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_OTHER);
        hipLaunchKernelGGL(wq_direct_kernel, dim3((unsigned)((n + WQ_DT - 1) / WQ_DT)), dim3(WN_THREADS), 0, c->stream, wc, g, mp, st,
                           sp.nan_missing, d_out);
        HIP_TRY(hipGetLastError());
        c->timings.algorithmic_bytes = 2 * (int64_t)dbytes + (has_null ? (int64_t)mbytes : 0);
    } else {
        // ---- the order: the sort's workspace, the permutation and this path's buffers in one arena, sized up front ----
        const KeyDesc key{cv.data, cv.mask, nullptr, col->dtype};
        int64_t *perm = nullptr;
        ST_TRY(sort_order_device(c, &key, 1, nullptr, nullptr, 0, n, nullptr, wq_workspace(n), &perm));
        const int64_t sort_bytes = c->timings.algorithmic_bytes;
        const int L = wq_levels(n);
        const int64_t n_words = n / 64 + 1;
        const size_t tiles = (size_t)(n_words + WQ_TILE_WORDS - 1) / WQ_TILE_WORDS;
        const bool nan_vector = !sp.nan_missing && !i64;
        uint32_t *ra = c->work.take<uint32_t>((size_t)n), *rb = c->work.take<uint32_t>((size_t)n);
        double *sorted_val = c->work.take<double>((size_t)n);
        WqWord *words = c->work.take<WqWord>(((size_t)L + 2) * (size_t)n_words);
        uint32_t *tile_ones = c->work.take<uint32_t>(tiles), *carry = c->work.take<uint32_t>(tiles), *zeros = c->work.take<uint32_t>(64);
        if (!perm || !ra || !rb || !sorted_val || !words || !tile_ones || !carry || !zeros)
            return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (window_quantile)");
        WqWord *incl = words + (size_t)L * n_words, *nanv = nan_vector ? incl + n_words : nullptr;
        {
            PhaseTimer pt(c, PANDRS_HIP_PHASE_BUILD);
            hipLaunchKernelGGL(wq_rank_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const int64_t *)perm, wc, ra, sorted_val);
            HIP_TRY(hipGetLastError());
            for (int l = 0; l < L; l++) {
                ST_TRY(wq_vector(c, WqRankBit{ra, L - 1 - l}, n, n_words, tile_ones, carry, zeros + l, words + (size_t)l * n_words,
                                 l + 1 < L ? rb : nullptr));           // the last level's order is read by nobody
                std::swap(ra, rb);
            }
            ST_TRY(wq_vector(c, WqInclBit{wc, sp.nan_missing}, n, n_words, tile_ones, carry, zeros + L, incl, nullptr));
            if (nanv) ST_TRY(wq_vector(c, WqNanBit{wc}, n, n_words, tile_ones, carry, zeros + L + 1, nanv, nullptr));
        }
        {
            PhaseTimer pt(c, PANDRS_HIP_PHASE_PROBE);
            const WqQuery Q{words, zeros, incl, nanv, sorted_val, g, n_words, mp, L, rolling ? 0 : 1, st};
            hipLaunchKernelGGL(wq_query_kernel, dim3((unsigned)((n + WN_THREADS - 1) / WN_THREADS)), dim3(WN_THREADS), 0, c->stream, Q, d_out);
            HIP_TRY(hipGetLastError());
        }
        // the ranks: the permutation in, ranks and cells out; a level: the ranks twice in, once out, and its words; the query's look-ups
        c->timings.algorithmic_bytes = sort_bytes + (int64_t)n * (8 + 8 + 4 + 8) + (int64_t)L * ((int64_t)n * 12 + n_words * 16) +
                                       (int64_t)n * (2 * L + 2) * 16 + (int64_t)dbytes;
    }
    ST_TRY(stg.copy_back(dbytes));
    ST_TRY(timings_end(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace pandrs
