// topk.hip — the first k rows of one numeric column in descending or ascending order, and the rows of its extremes, behind
// PandasCompatExt::nlargest / nsmallest / idxmax / idxmin (reference src/dataframe/pandas_compat/functions.rs:159-192),
// gfx950, wave64.  The order is pandrs_hip_sort_indices' for that one key: numbers by value, ties in row order, then the NaN
// rows, then the null rows.  No sort of the column: a SELECT of the k-th value, a compaction of what beats it, and a sort of
// fewer than k rows.  Every hand-off between workgroups is a kernel boundary; no workgroup waits for another.
// 1. Census (tk_census_kernel, tk_plan_kernel): one stream of 16-byte loads over the column and its mask counts the numbers
//    (m), the NaN and the null cells and keeps the smallest order-preserving code (enc_f64 with -0.0 folded onto 0.0 /
//    enc_i64) with the FIRST row that holds it and the largest with the LAST (Iterator::min_by / max_by): that pair is
//    pandrs_hip_arg_extreme's whole answer.  One workgroup folds the partials and splits the output into kn = min(k, m)
//    numbers, kN NaN rows and kU null rows.
// 2. Select (tk_select_kernel + tk_pick_kernel per digit): single-rank MSD radix select, 8-bit digits, of rank kn - 1 over
//    d = code - min (LARGEST: max - code).  A row whose higher digits equal the prefix chosen so far counts its digit in the
//    workgroup's LDS histogram, equal digits of a wave first folded by ballot; one workgroup scans the 256 counts and
//    narrows the rank.  The first stream also ORs d, so a digit in which no row has a bit set costs no stream.  The host
//    enqueues all eight passes; a pass beyond the width returns at once.  kn == m: every number is taken, no select.
// 3. Compact (tk_count_kernel, tk_scan_kernel, tk_place_kernel), reduce-then-scan: per tile the rows better than the
//    threshold T, equal to it, NaN and null are counted (four 16-bit fields of one word), one workgroup scans the tile counts
//    (the total of "better" is s, the tie quota q = kn - s), and a last stream, which skips every tile that has nothing to
//    give, ranks the rows of a tile with wave ballots and mbcnt, so that every class keeps row order: a better row goes to
//    the candidate list (cell and row number, position = rank), an equal row with rank < q to its final slot s + rank, NaN
//    rows with rank < kN to kn + rank, null rows with rank < kU to kn + kN + rank.
// 4. Order (sort_order_device, tk_gather_kernel): s reaches the host (the one read-back of its own; the nested sort makes two), the s < k candidate
//    cells are ordered by the stable sort of sort.hip in the wanted direction, and the candidates' row numbers are gathered
//    through its permutation into out[0, s).
// 5. Cut-over: from k * TK_CUT_DEN >= n_rows * TK_CUT_NUM on the select buys nothing: the whole column is sorted and the
//    first k entries of the permutation are the answer (the census still runs, for the number count).
//
// Resources (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage; no kernel spills to scratch):
//   kernel            VGPRs  LDS bytes      kernel            VGPRs  LDS bytes
//   tk_census_kernel     86        224      tk_count_kernel      72         32
//   tk_plan_kernel       40        224      tk_scan_kernel       20      16384
//   tk_select_kernel     68       1024      tk_place_kernel      64       1536
//   tk_pick_kernel       16         68      tk_gather_kernel      6          0
#include "engine.hpp"

#include <algorithm>

namespace pandrs {

constexpr int TK_THREADS = 256;                          // 4 waves
constexpr int TK_LOADS = 4;                              // 16-byte loads in flight per thread
constexpr int TK_TILE = TK_THREADS * TK_LOADS * 2;       // 2048 rows per workgroup iteration: topk_tile_rows of pandrs_hip.h
constexpr int TK_RPT = TK_TILE / TK_THREADS;             // rows per thread of a tile in the placing kernel
constexpr int TK_WORDS = TK_TILE / 64;                   // ballot words per tile
constexpr int TK_BLOCKS_PER_CU = 4;                      // topk_blocks_per_cu of pandrs_hip.h
constexpr int TK_DIGIT = 8, TK_BINS = 1 << TK_DIGIT;
constexpr int TK_MAX_PASSES = 64 / TK_DIGIT;
constexpr int TK_PEEL = 4;                               // digits a wave folds by ballot before plain atomics
constexpr int TK_SCAN_THREADS = 1024;
constexpr int64_t TK_CUT_NUM = 1, TK_CUT_DEN = 5;        // topk_cutover of pandrs_hip.h: k / n_rows from which the sort answers
enum : int { TK_BETTER = 0, TK_EQUAL = 1, TK_NAN = 2, TK_NULL = 3, TK_CLASSES = 4, TK_NONE = 4 };
static_assert(TK_BINS == TK_THREADS, "a thread owns a digit");
static_assert(TK_TILE < (1 << 16), "a tile's four class counts travel as 16-bit fields of one word");

struct TkCol {
    const uint64_t *data;     // 8-byte aligned
    const uint8_t *null;      // LSB-first, 1 = null, any byte offset
    int64_t n;
    int i64;
};

struct TkPart {               // one workgroup's census; mn / mx and their rows are meaningful when num > 0
    uint64_t num, nan, nul, mn, mx;
    int64_t mn_row, mx_row;
};

struct TkState {
    uint64_t num, nan, nul, mn, mx;       // the census of the column
    int64_t mn_row, mx_row;               // first row of the smallest number, last row of the largest
    uint64_t kn, kN, kU;                  // numbers, NaN rows and null rows of the output
    uint64_t prefix, rank;                // the select: digits of d chosen so far, the rank among the rows that share them
    uint64_t vary;                        // OR of d over the numbers, known after the first digit stream
    uint64_t s, q;                        // rows better than the threshold, tie quota (after the scan)
    int32_t n_pass, take_all, largest, pad;
};

__device__ __forceinline__ bool tk_is_nan(uint64_t b, int i64) { return !i64 && (b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull; }
// order-preserving code of a number; -0.0 == 0.0 (partial_cmp), as sort_sortable
__device__ __forceinline__ uint64_t tk_code(uint64_t b, int i64) {
    if (i64) return enc_i64((int64_t)b);
    if (b == 0x8000000000000000ull) b = 0;
    return enc_f64(__longlong_as_double((long long)b));
}

// f(bits, row, in, null) for every row slot of this workgroup's tiles, called by all threads together (f may ballot); `in`
// is false past the last row.  A thread meets its rows in ascending row order.  A data pointer that is 8 bytes off a
// 16-byte boundary takes its row pairs as two 8-byte loads.
template <class F>
__device__ __forceinline__ void tk_stream(const TkCol &c, F &&f) {
    const bool aligned = (reinterpret_cast<uintptr_t>(c.data) & 15) == 0;
    const int64_t tiles = (c.n + TK_TILE - 1) / TK_TILE;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t r0 = t * TK_TILE + 2 * (int64_t)threadIdx.x;
        uint64_t v[TK_LOADS][2];
        uint32_t in[TK_LOADS], nul[TK_LOADS];
#pragma unroll
        for (int k = 0; k < TK_LOADS; k++) {
            const int64_t r = r0 + (int64_t)k * 2 * TK_THREADS;          // even: both rows' mask bits lie in one byte
            in[k] = 0;
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
            nul[k] = (c.null && in[k]) ? ((uint32_t)c.null[r >> 3] >> (r & 7)) & in[k] : 0;
        }
#pragma unroll
        for (int k = 0; k < TK_LOADS; k++) {
            const int64_t r = r0 + (int64_t)k * 2 * TK_THREADS;
            f(v[k][0], r, (in[k] & 1) != 0, (nul[k] & 1) != 0);
            f(v[k][1], r + 1, (in[k] & 2) != 0, (nul[k] & 2) != 0);
        }
    }
}

// (code, row) pairs fold as pairs, so the result does not depend on the order of the folds
__device__ __forceinline__ void tk_merge(TkPart &a, const TkPart &b) {
    if (b.num) {
        if (!a.num || b.mn < a.mn || (b.mn == a.mn && b.mn_row < a.mn_row)) { a.mn = b.mn; a.mn_row = b.mn_row; }
        if (!a.num || b.mx > a.mx || (b.mx == a.mx && b.mx_row > a.mx_row)) { a.mx = b.mx; a.mx_row = b.mx_row; }
    }
    a.num += b.num; a.nan += b.nan; a.nul += b.nul;
}

// the workgroup's census; the result is valid in thread 0
__device__ __forceinline__ TkPart tk_block_part(TkPart p, TkPart *sh) {
    for (int o = 32; o >= 1; o >>= 1) {
        TkPart b;
        b.num = __shfl_down(p.num, o, 64); b.nan = __shfl_down(p.nan, o, 64); b.nul = __shfl_down(p.nul, o, 64);
        b.mn = __shfl_down(p.mn, o, 64); b.mx = __shfl_down(p.mx, o, 64);
        b.mn_row = __shfl_down(p.mn_row, o, 64); b.mx_row = __shfl_down(p.mx_row, o, 64);
        tk_merge(p, b);                                   // (lanes whose partner lies past the wave fold themselves: not lane 0's tree)
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = p;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < TK_THREADS / 64; w++) tk_merge(p, sh[w]);
    return p;
}

// ---- 1. census ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TK_THREADS) void tk_census_kernel(TkCol c, TkPart *part) {
    __shared__ TkPart sh[TK_THREADS / 64];
    TkPart p{0, 0, 0, 0, 0, -1, -1};
    tk_stream(c, [&](uint64_t b, int64_t row, bool in, bool nul) {
        if (!in) return;
        if (nul) { p.nul++; return; }
        if (tk_is_nan(b, c.i64)) { p.nan++; return; }
        const uint64_t e = tk_code(b, c.i64);
        if (!p.num || e < p.mn) { p.mn = e; p.mn_row = row; }             // min_by keeps the first of equals
        if (!p.num || e >= p.mx) { p.mx = e; p.mx_row = row; }            // max_by keeps the last
        p.num++;
    });
    p = tk_block_part(p, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = p;
}

__global__ __launch_bounds__(TK_THREADS) void tk_plan_kernel(const TkPart *part, int n_part, uint64_t k, int largest, TkState *st) {
    __shared__ TkPart sh[TK_THREADS / 64];
    TkPart p{0, 0, 0, 0, 0, -1, -1};
    for (int i = threadIdx.x; i < n_part; i += TK_THREADS) tk_merge(p, part[i]);
    p = tk_block_part(p, sh);
    if (threadIdx.x != 0) return;
    st->num = p.num; st->nan = p.nan; st->nul = p.nul; st->mn = p.mn; st->mx = p.mx;
    st->mn_row = p.mn_row; st->mx_row = p.mx_row;
    const uint64_t kn = k < p.num ? k : p.num;
    const uint64_t kN = k - kn < p.nan ? k - kn : p.nan;
    const uint64_t kU = k - kn - kN < p.nul ? k - kn - kN : p.nul;
    st->kn = kn; st->kN = kN; st->kU = kU;
    const uint64_t span = p.num ? p.mx - p.mn : 0;
    const int width = span ? 64 - __clzll((long long)span) : 0;
    st->take_all = kn == p.num;                          // every number is taken: all of them are "better", none ties
    st->largest = largest;
    st->n_pass = (kn && !st->take_all) ? (width + TK_DIGIT - 1) / TK_DIGIT : 0;     // width 0: every number equals the threshold
    st->prefix = 0;
    st->rank = kn ? kn - 1 : 0;
    st->vary = 0;
    st->s = st->q = 0;
    st->pad = 0;
}

// ---- 2. select ------------------------------------------------------------------------------------------------------------
// a digit below the first in which no row has a bit set: every row's digit is 0, so no stream is needed
__device__ __forceinline__ bool tk_digit_is_zero(const TkState *st, int pass) {
    return pass > 0 && pass < st->n_pass && ((st->vary >> (TK_DIGIT * (st->n_pass - 1 - pass))) & (TK_BINS - 1)) == 0;
}

// lanes holding the same digit as the first pending lane add their number in one LDS atomic
__device__ __forceinline__ void tk_hist_add(uint32_t *h, bool m, uint32_t key) {
    uint64_t todo = __ballot(m);
    const uint32_t lane = threadIdx.x & 63;
    for (int round = 0; todo && round < TK_PEEL; round++) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint32_t k0 = __shfl(key, leader, 64);
        const uint64_t same = __ballot(m && key == k0) & todo;
        if (lane == (uint32_t)leader) atomicAdd(&h[k0], (uint32_t)__popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1) atomicAdd(&h[key], 1u);
}

__global__ __launch_bounds__(TK_THREADS) void tk_select_kernel(TkCol c, const TkState *st, int pass, uint32_t *hist, unsigned long long *vary) {
    __shared__ uint32_t h[TK_BINS];
    const int n_pass = st->n_pass;
    if (pass >= n_pass || tk_digit_is_zero(st, pass)) return;
    const int shift = TK_DIGIT * (n_pass - 1 - pass), hs = shift + TK_DIGIT;
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t prefix = st->prefix, base = st->largest ? st->mx : st->mn;
    const int largest = st->largest;
    uint64_t d_or = 0;
    tk_stream(c, [&](uint64_t b, int64_t, bool in, bool nul) {
        bool m = false;
        uint32_t key = 0;
        if (in && !nul && !tk_is_nan(b, c.i64)) {
            const uint64_t e = tk_code(b, c.i64), d = largest ? base - e : e - base;
            d_or |= d;
            if ((hs >= 64 ? 0ull : d >> hs) == prefix) { m = true; key = (uint32_t)(d >> shift) & (TK_BINS - 1); }
        }
        tk_hist_add(h, m, key);
    });
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
    if (pass == 0) {                                     // which lower digits vary at all
        for (int o = 32; o >= 1; o >>= 1) d_or |= __shfl_down(d_or, o, 64);
        if ((threadIdx.x & 63) == 0 && d_or) atomicOr(vary, (unsigned long long)d_or);
    }
}

__global__ __launch_bounds__(TK_THREADS) void tk_pick_kernel(TkState *st, int pass, uint32_t *hist) {
    __shared__ uint32_t wave_tot[17];
    if (pass >= st->n_pass) return;
    if (tk_digit_is_zero(st, pass)) {                    // the chosen digit is 0; the rank stays
        if (threadIdx.x == 0) st->prefix <<= TK_DIGIT;
        return;
    }
    const uint64_t r = st->rank, prefix = st->prefix;
    const uint32_t v = hist[threadIdx.x];
    hist[threadIdx.x] = 0;                               // armed for the next pass
    __syncthreads();                                     // every thread holds the old rank before one of them writes the new
    const uint32_t ex = block_exclusive_scan<TK_THREADS>(v, wave_tot, nullptr);
    if (v && r >= ex && r < (uint64_t)ex + v) {
        st->prefix = (prefix << TK_DIGIT) | threadIdx.x;
        st->rank = r - ex;
    }
}

// ---- 3. compact -----------------------------------------------------------------------------------------------------------
struct TkSel {
    uint64_t base, T;
    int largest, take_all;
};
__device__ __forceinline__ TkSel tk_sel(const TkState *st) {
    return TkSel{st->largest ? st->mx : st->mn, st->prefix, st->largest, st->take_all};
}
__device__ __forceinline__ int tk_class(const TkSel &s, int i64, uint64_t b, bool nul) {
    if (nul) return TK_NULL;
    if (tk_is_nan(b, i64)) return TK_NAN;
    const uint64_t e = tk_code(b, i64), d = s.largest ? s.base - e : e - s.base;
    if (s.take_all || d < s.T) return TK_BETTER;
    return d == s.T ? TK_EQUAL : TK_NONE;
}

// counts[cls * tiles + t] = rows of class cls in tile t
__global__ __launch_bounds__(TK_THREADS) void tk_count_kernel(TkCol c, const TkState *st, int64_t tiles, uint32_t *counts) {
    __shared__ uint64_t sh[TK_THREADS / 64];
    const TkSel sel = tk_sel(st);
    uint64_t acc = 0;                                    // four 16-bit fields
    int slot = 0;                                        // tk_stream hands over 2 * TK_LOADS row slots per tile
    int64_t t = blockIdx.x;
    tk_stream(c, [&](uint64_t b, int64_t, bool in, bool nul) {
        if (in) {
            const int cl = tk_class(sel, c.i64, b, nul);
            if (cl < TK_CLASSES) acc += 1ull << (16 * cl);
        }
        if (++slot < 2 * TK_LOADS) return;
        for (int o = 32; o >= 1; o >>= 1) acc += __shfl_down(acc, o, 64);
        __syncthreads();                                 // the previous tile's partials are consumed
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x < TK_CLASSES) {
            uint64_t a = 0;
            for (int w = 0; w < TK_THREADS / 64; w++) a += sh[w];
            counts[(int64_t)threadIdx.x * tiles + t] = (uint32_t)(a >> (16 * threadIdx.x)) & 0xFFFFu;
        }
        acc = 0;
        slot = 0;
        t += gridDim.x;
    });
}

// offs = the exclusive scan of every class's tile counts; one workgroup, thread i owns a contiguous range of tiles
__global__ __launch_bounds__(TK_SCAN_THREADS) void tk_scan_kernel(const uint32_t *counts, uint32_t *offs, int64_t tiles, TkState *st) {
    __shared__ uint32_t sh[TK_CLASSES][TK_SCAN_THREADS];
    const int tid = threadIdx.x;
    const int64_t per = (tiles + TK_SCAN_THREADS - 1) / TK_SCAN_THREADS;
    const int64_t beg = tid * per < tiles ? tid * per : tiles, end = beg + per < tiles ? beg + per : tiles;
    for (int cl = 0; cl < TK_CLASSES; cl++) {
        uint32_t sum = 0;                                // (a class holds fewer than 2^32 rows: n_rows < 2^32)
        for (int64_t t = beg; t < end; t++) sum += counts[cl * tiles + t];
        sh[cl][tid] = sum;
    }
    __syncthreads();
    for (int o = 1; o < TK_SCAN_THREADS; o <<= 1) {      // inclusive over threads <= tid
        uint32_t a[TK_CLASSES];
        for (int cl = 0; cl < TK_CLASSES; cl++) a[cl] = tid >= o ? sh[cl][tid - o] : 0;
        __syncthreads();
        for (int cl = 0; cl < TK_CLASSES; cl++) sh[cl][tid] += a[cl];
        __syncthreads();
    }
    for (int cl = 0; cl < TK_CLASSES; cl++) {
        uint32_t run = tid ? sh[cl][tid - 1] : 0;
        for (int64_t t = beg; t < end; t++) {
            offs[cl * tiles + t] = run;
            run += counts[cl * tiles + t];
        }
    }
    if (tid == TK_SCAN_THREADS - 1) {
        const uint64_t s = sh[TK_BETTER][tid];
        st->s = s;
        st->q = st->kn >= s ? st->kn - s : 0;            // (the select leaves s < kn, or s == kn when every number is taken)
    }
}

// Rows of a tile in row order: thread tid owns rows r * TK_THREADS + tid, so wave w's ballot at step r is the tile's word
// r * 4 + w.  cap = the entries out, cand_cell and cand_row hold: no store lands at or beyond it.
__global__ __launch_bounds__(TK_THREADS) void tk_place_kernel(TkCol c, const TkState *st, const uint32_t *counts, const uint32_t *offs,
                                                               int64_t tiles, uint64_t cap, uint64_t *cand_cell, int64_t *cand_row, int64_t *out) {
    __shared__ uint64_t bal[TK_WORDS][TK_CLASSES];
    __shared__ uint32_t pre[TK_WORDS][TK_CLASSES];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const TkSel sel = tk_sel(st);
    const uint64_t s = st->s, q = st->q, kn = st->kn, kN = st->kN, kU = st->kU;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        uint64_t off[TK_CLASSES];
        bool need = false;
        for (int cl = 0; cl < TK_CLASSES; cl++) {
            off[cl] = offs[cl * tiles + t];
            const uint64_t quota = cl == TK_BETTER ? s : (cl == TK_EQUAL ? q : (cl == TK_NAN ? kN : kU));
            need = need || (counts[cl * tiles + t] != 0 && off[cl] < quota);
        }
        if (!need) continue;                             // (uniform: the tile gives nothing to the output)
        __syncthreads();                                 // the previous tile's words are consumed
        uint64_t cell[TK_RPT];
        int cls[TK_RPT];
#pragma unroll
        for (int r = 0; r < TK_RPT; r++) {               // (a uniform loop: the ballots see every lane)
            const int64_t row = t * TK_TILE + r * TK_THREADS + tid;
            cell[r] = 0;
            cls[r] = TK_NONE;
            if (row < c.n) {
                cell[r] = c.data[row];
                cls[r] = tk_class(sel, c.i64, cell[r], c.null && bit_at(c.null, row));
            }
#pragma unroll
            for (int cl = 0; cl < TK_CLASSES; cl++) {
                const uint64_t m = __ballot(cls[r] == cl);
                if (lane == 0) bal[r * (TK_THREADS / 64) + wave][cl] = m;
            }
        }
        __syncthreads();
        if (tid < TK_CLASSES) {
            uint32_t run = 0;
            for (int j = 0; j < TK_WORDS; j++) { pre[j][tid] = run; run += (uint32_t)__popcll(bal[j][tid]); }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < TK_RPT; r++) {
            const int cl = cls[r];
            if (cl >= TK_CLASSES) continue;
            const int64_t row = t * TK_TILE + r * TK_THREADS + tid;
            const uint32_t j = r * (TK_THREADS / 64) + wave;
            const uint64_t m = bal[j][cl];
            const uint64_t g = off[cl] + pre[j][cl] + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (cl == TK_BETTER) {
                if (g < s && g < cap) { cand_cell[g] = cell[r]; cand_row[g] = row; }
            } else if (cl == TK_EQUAL) {
                if (g < q && s + g < cap) out[s + g] = row;
            } else if (cl == TK_NAN) {
                if (g < kN && kn + g < cap) out[kn + g] = row;
            } else {
                if (g < kU && kn + kN + g < cap) out[kn + kN + g] = row;
            }
        }
    }
}

// ---- 4. order -------------------------------------------------------------------------------------------------------------
// out[j] = the row of the candidate that the sort put at position j (perm == nullptr: a single candidate)
__global__ void tk_gather_kernel(const int64_t *perm, const int64_t *cand_row, int64_t s, int64_t *out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= s) return;
    const int64_t p = perm ? perm[j] : j;
    if ((uint64_t)p < (uint64_t)s) out[j] = cand_row[p];                 // (a permutation holds positions only; a guard, not a path)
}

// ---- host side ------------------------------------------------------------------------------------------------------------
namespace {

int tk_grid(const pandrs_hip_ctx *c, int64_t n_rows) {
    const int64_t tiles = (n_rows + TK_TILE - 1) / TK_TILE;
    return (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)c->n_cu * TK_BLOCKS_PER_CU, tiles));
}

struct TkCommon {             // what both entry points set up: the staged column and the census buffers
    TkCol col;
    TkPart *part;
    TkState *st;
    int grid;
};

// census + plan, enqueued; *st is complete when the stream reaches the next kernel
void tk_census(pandrs_hip_ctx *c, const TkCommon &t, uint64_t k, int largest) {
    hipLaunchKernelGGL(tk_census_kernel, dim3(t.grid), dim3(TK_THREADS), 0, c->stream, t.col, t.part);
    hipLaunchKernelGGL(tk_plan_kernel, dim3(1), dim3(TK_THREADS), 0, c->stream, (const TkPart *)t.part, t.grid, k, largest, t.st);
}

int32_t tk_read_state(pandrs_hip_ctx *c, const TkState *d_st, TkState *h_st) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->pinned, d_st, sizeof(TkState), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::memcpy(h_st, c->pinned, sizeof(TkState));
    return 0;
}

}  // namespace

int32_t topk_entry(pandrs_hip_ctx *c, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows, int64_t k, int32_t direction,
                   int32_t out_mem_space, int64_t *out_rows, int64_t *out_count, int64_t *out_n_numbers) {
    if (!c || !col || !out_count || !out_n_numbers || n_rows < 0 || k < 0)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "topk: bad arguments");
    ST_TRY(check_mem_space("topk", mem_space, out_mem_space));
    if (direction != PANDRS_HIP_TOPK_LARGEST && direction != PANDRS_HIP_TOPK_SMALLEST)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "topk: direction %d is not a pandrs_hip_topk_direction", direction);
    if (col->dtype != PANDRS_HIP_I64 && col->dtype != PANDRS_HIP_F64)
        return fail(PANDRS_HIP_ERR_TYPE_MISMATCH, "topk: the column has dtype %d, expected I64 or F64", col->dtype);
    if (n_rows >= (int64_t(1) << 32))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "topk: %lld rows; one call takes fewer than 2^32", (long long)n_rows);
    const int64_t kk = std::min(k, n_rows);
    if (kk > 0 && (!col->data || !out_rows)) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "topk: null column data or output");
    *out_count = *out_n_numbers = 0;
    if (kk == 0) return 0;
    std::lock_guard<std::mutex> lock(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    timings_begin(c);

    ColView cv{col->data, col->null_mask};
    int64_t *d_out = out_rows;
    Stager stg{c, mem_space, out_mem_space};
    if (const size_t need = stg.col_size(*col, n_rows) + stg.out_size(out_rows, (size_t)kk * 8)) {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_STAGE_IN);
        ST_TRY(stg.reserve(need));
        cv = stg.col(*col, n_rows);
        d_out = stg.out(out_rows, (size_t)kk * 8);
        if (stg.status) return stg.status;
    }
    if ((reinterpret_cast<uintptr_t>(cv.data) | reinterpret_cast<uintptr_t>(d_out)) & 7)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "topk: the column and out_rows must be 8-byte aligned");

    // ---- workspace, sized up front: the census partials, the state, the digit counts; below the cut-over the tile counts and
    // offsets, the candidates and the sort of kk rows; above it the sort of the column ----
    const bool by_sort = c->opt.topk_path > 0 || (c->opt.topk_path == 0 && kk * TK_CUT_DEN >= n_rows * TK_CUT_NUM);
    const int64_t tiles = (n_rows + TK_TILE - 1) / TK_TILE;
    TkCommon t{};
    t.col = TkCol{static_cast<const uint64_t *>(cv.data), cv.mask, n_rows, col->dtype == PANDRS_HIP_I64 ? 1 : 0};
    t.grid = tk_grid(c, n_rows);
    const size_t n_tc = (size_t)TK_CLASSES * (size_t)tiles;
    ST_TRY(c->topk.ensure(Arena::padded((size_t)t.grid * sizeof(TkPart)) + Arena::padded(sizeof(TkState)) + Arena::padded(TK_BINS * 4) +
                          (by_sort ? 0 : 2 * Arena::padded(n_tc * 4) + 2 * Arena::padded((size_t)kk * 8)) + 4096, c->stream));
    t.part = c->topk.take<TkPart>((size_t)t.grid);
    t.st = c->topk.take<TkState>(1);
    uint32_t *hist = c->topk.take<uint32_t>(TK_BINS);
    if (!t.part || !t.st || !hist) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (topk)");
    const int32_t asc = direction == PANDRS_HIP_TOPK_SMALLEST ? 1 : 0;
    TkState hs{};
    int64_t passes = 0, alg = 0;
    const int64_t stream_bytes = n_rows * 8 + (cv.mask ? (n_rows + 7) / 8 : 0);

    if (by_sort) {
        {
            PhaseTimer pt(c, PANDRS_HIP_PHASE_OTHER);
            tk_census(c, t, (uint64_t)kk, asc ? 0 : 1);
            HIP_TRY(hipGetLastError());
        }
        const KeyDesc key{cv.data, cv.mask, nullptr, col->dtype};
        int64_t *perm = nullptr;
        ST_TRY(sort_order_device(c, &key, 1, &asc, nullptr, 0, n_rows, nullptr, 0, &perm));
        if (!perm) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (topk)");
        HIP_TRY(hipMemcpyAsync(d_out, perm, (size_t)kk * 8, hipMemcpyDeviceToDevice, c->stream));
        ST_TRY(tk_read_state(c, t.st, &hs));
        passes = c->timings.n_partitions;
        alg = c->timings.algorithmic_bytes + stream_bytes + kk * 16;
    } else {
        uint32_t *counts = c->topk.take<uint32_t>(n_tc), *offs = c->topk.take<uint32_t>(n_tc);
        uint64_t *cand_cell = c->topk.take<uint64_t>((size_t)kk);
        int64_t *cand_row = c->topk.take<int64_t>((size_t)kk);
        if (!counts || !offs || !cand_cell || !cand_row) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (topk)");
        // the candidates hold neither NaN nor null: their code fits one word; + the permutation
        ST_TRY(c->work.ensure(sort_order_workspace(c, kk, 1) + Arena::padded((size_t)kk * 8), c->stream));
        {
            PhaseTimer pt(c, PANDRS_HIP_PHASE_OTHER);
            HIP_TRY(hipMemsetAsync(hist, 0, TK_BINS * 4, c->stream));
            tk_census(c, t, (uint64_t)kk, asc ? 0 : 1);
            for (int pass = 0; pass < TK_MAX_PASSES; pass++) {
                // (vary aliases st->vary: pass 0 writes it and never reads it, later passes read it after a kernel boundary)
                hipLaunchKernelGGL(tk_select_kernel, dim3(t.grid), dim3(TK_THREADS), 0, c->stream, t.col, (const TkState *)t.st, pass, hist,
                                   reinterpret_cast<unsigned long long *>(&t.st->vary));
                hipLaunchKernelGGL(tk_pick_kernel, dim3(1), dim3(TK_THREADS), 0, c->stream, t.st, pass, hist);
            }
            HIP_TRY(hipGetLastError());
        }
        {
            PhaseTimer pt(c, PANDRS_HIP_PHASE_SCATTER);
            hipLaunchKernelGGL(tk_count_kernel, dim3(t.grid), dim3(TK_THREADS), 0, c->stream, t.col, (const TkState *)t.st, tiles, counts);
            hipLaunchKernelGGL(tk_scan_kernel, dim3(1), dim3(TK_SCAN_THREADS), 0, c->stream, (const uint32_t *)counts, offs, tiles, t.st);
            hipLaunchKernelGGL(tk_place_kernel, dim3(t.grid), dim3(TK_THREADS), 0, c->stream, t.col, (const TkState *)t.st, (const uint32_t *)counts,
                               (const uint32_t *)offs, tiles, (uint64_t)kk, cand_cell, cand_row, d_out);
        }
        ST_TRY(tk_read_state(c, t.st, &hs));                // s sizes the sort: the one read-back of top-k's own
        const int64_t s = (int64_t)hs.s;
        if (hs.s > hs.kn || hs.s + hs.q != hs.kn || hs.kn + hs.kN + hs.kU != (uint64_t)kk)
            return fail(PANDRS_HIP_ERR_COMPUTATION, "topk: the selection does not add up (%llu better + %llu ties for %llu numbers)",
                        (unsigned long long)hs.s, (unsigned long long)hs.q, (unsigned long long)hs.kn);
        for (int pass = 0; pass < hs.n_pass; pass++)
            passes += pass == 0 || ((hs.vary >> (TK_DIGIT * (hs.n_pass - 1 - pass))) & (TK_BINS - 1)) != 0;
        alg = stream_bytes * (2 + passes) + kk * 8 + s * 16;
        if (s > 0) {
            int64_t *perm = nullptr;
            if (s > 1) {
                const KeyDesc key{cand_cell, nullptr, nullptr, col->dtype};
                ST_TRY(sort_order_device(c, &key, 1, &asc, nullptr, 0, s, nullptr, 0, &perm));
                if (!perm) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (topk)");
                alg += c->timings.algorithmic_bytes;
            }
            PhaseTimer pt(c, PANDRS_HIP_PHASE_GATHER);
            hipLaunchKernelGGL(tk_gather_kernel, dim3((unsigned)((s + 255) / 256)), dim3(256), 0, c->stream, (const int64_t *)perm,
                               (const int64_t *)cand_row, s, d_out);
            HIP_TRY(hipGetLastError());
            alg += s * 24;
        }
    }
    c->timings.algorithmic_bytes = alg;
    c->timings.n_partitions = passes;
    ST_TRY(stg.copy_back((size_t)kk * 8));
    ST_TRY(timings_end(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out_count = kk;
    *out_n_numbers = (int64_t)std::min<uint64_t>((uint64_t)kk, hs.num);
    return 0;
}

int32_t arg_extreme_entry(pandrs_hip_ctx *c, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows, int64_t *out_rows,
                          int32_t *out_found) {
    if (!c || !col || !out_rows || !out_found || n_rows < 0 || (n_rows > 0 && !col->data))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "arg_extreme: bad arguments");
    ST_TRY(check_mem_space("arg_extreme", mem_space));
    if (col->dtype != PANDRS_HIP_I64 && col->dtype != PANDRS_HIP_F64)
        return fail(PANDRS_HIP_ERR_TYPE_MISMATCH, "arg_extreme: the column has dtype %d, expected I64 or F64", col->dtype);
    if (n_rows >= (int64_t(1) << 32))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "arg_extreme: %lld rows; one call takes fewer than 2^32", (long long)n_rows);
    *out_found = 0;
    if (n_rows == 0) return 0;
    std::lock_guard<std::mutex> lock(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    timings_begin(c);
    ColView cv{col->data, col->null_mask};
    Stager stg{c, mem_space};
    if (const size_t need = stg.col_size(*col, n_rows)) {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_STAGE_IN);
        ST_TRY(stg.reserve(need));
        cv = stg.col(*col, n_rows);
        if (stg.status) return stg.status;
    }
    if (reinterpret_cast<uintptr_t>(cv.data) & 7) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "arg_extreme: the column must be 8-byte aligned");
    TkCommon t{};
    t.col = TkCol{static_cast<const uint64_t *>(cv.data), cv.mask, n_rows, col->dtype == PANDRS_HIP_I64 ? 1 : 0};
    t.grid = tk_grid(c, n_rows);
    ST_TRY(c->topk.ensure(Arena::padded((size_t)t.grid * sizeof(TkPart)) + Arena::padded(sizeof(TkState)) + 4096, c->stream));
    t.part = c->topk.take<TkPart>((size_t)t.grid);
    t.st = c->topk.take<TkState>(1);
    if (!t.part || !t.st) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (arg_extreme)");
    {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_OTHER);
        tk_census(c, t, 0, 0);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(c->pinned, t.st, sizeof(TkState), hipMemcpyDeviceToHost, c->stream));
    c->timings.algorithmic_bytes = n_rows * 8 + (cv.mask ? (n_rows + 7) / 8 : 0);
    ST_TRY(timings_end(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    TkState hs;
    std::memcpy(&hs, c->pinned, sizeof hs);
    if (hs.num) { out_rows[0] = hs.mn_row; out_rows[1] = hs.mx_row; *out_found = 1; }
    return 0;
}

}  // namespace pandrs
