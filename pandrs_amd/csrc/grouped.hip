// grouped.hip — running folds, lags and the row number of one numeric column WITHIN the groups the context retains from
// pandrs_hip_groupby_indices (c->gr: rows[], offsets[] in CSR form), behind GroupBy::cumsum / cummax / cummin / cumcount /
// row_number / shift / diff / pct_change, gfx950, wave64.  The contracts are pandrs_hip_cumulative's and pandrs_hip_lag's, read
// per group (include/pandrs_hip.h).
//
// The work runs in sorted-position order: position j holds row rows[j], group g is the contiguous positions offsets[g] ..
// offsets[g + 1], rows ascend inside it.  One bit per position says "a group starts here" (the head words, set from offsets[]
// by an atomicOr per group, the groups of one word and wave sharing one).  A 64-bit head word covers exactly the 64 positions one wave touches with one load, so it is
// wave-uniform and drives the cross-lane scan: a lane combines with the lane s below it only while no head lies between.
// The folds are a segmented reduce-then-apply over contiguous spans of whole tiles, the layout of cumulative.hip:
// 1. Reduce.  A workgroup gathers its span's cells through rows[] ONCE, leaves them (and their null bits as ballot words)
//    contiguous in the workspace, and folds the span into a summary: does it hold a head, and the fold of the cells after
//    its last head (of all its cells when it holds none).
// 2. Apply.  The prologue folds the summaries of the earlier spans back to the nearest one that holds a head: the carry.
//    The span's tiles are then scanned from the gathered cells and scattered to out[rows[j]].
// A group's prefix is only ever folded from its own cells: no global prefix is subtracted, nothing cancels across groups.
// Lag and ROW_NUMBER need the first position of the group per position: one ordinary max-scan of the head positions through
// the same tile scan (no head words: one segment) into a 32-bit array; a source position j' = j - periods is in the group iff
// 0 <= j' < n and start[j'] == start[j].  Lag reads the gathered cells, so the column is gathered once there too.
// Every hand-off between workgroups is a kernel boundary; no workgroup waits for another.
#include "cumulative.hpp"

#include <algorithm>

namespace pandrs {

#pragma clang fp contract(off)      // diff / pct_change are the reference's expressions, every operation rounded on its own

constexpr int GRP_THREADS = 256;                        // 4 waves
constexpr int GRP_WAVES = GRP_THREADS / 64;
constexpr int GRP_LOADS = 8;                            // 8-byte loads per lane and tile: one head word each
constexpr int GRP_WAVE_ROWS = GRP_LOADS * 64;           // positions one wave owns in a tile
constexpr int GRP_TILE = GRP_WAVES * GRP_WAVE_ROWS;     // 2048 positions: grouped_tile_rows of pandrs_hip.h
constexpr int GRP_BLOCKS_PER_CU = 4;                    // grouped_blocks_per_cu of pandrs_hip.h

struct GrpIn {                      // the retained grouping and the call's scratch, all in sorted-position order
    const int64_t *rows;            // [n] position -> row
    const uint64_t *heads;          // [tiles * GRP_TILE / 64] bit j: position j starts a group
    uint64_t *cells;                // [n] the gathered column
    uint64_t *nullw;                // [tiles * GRP_TILE / 64] the gathered null bits, one ballot per load
    uint32_t *start;                // [n] the first position of the position's group (lag, ROW_NUMBER)
    int64_t n;
};

struct GrpSpans {
    int64_t tiles, base, rem;       // span b holds base + (b < rem) tiles from tile b * base + min(b, rem)
    void *sum_v;                    // [grid] the fold of the span's cells after its last head
    uint32_t *sum_f;                // [grid] the span holds a head
};

struct GrpStart {                   // the max-scan of head positions: position 0 is a head and the identity at once
    using S = uint32_t;
    __device__ static S identity() { return 0; }
    __device__ static S combine(S a, S b) { return a > b ? a : b; }
};

__device__ __forceinline__ double grp_shfl_xor(double v, int m) { return __shfl_xor(v, m, 64); }
__device__ __forceinline__ uint32_t grp_shfl_xor(uint32_t v, int m) { return (uint32_t)__shfl_xor((int)v, m, 64); }
__device__ __forceinline__ uint64_t grp_upto(uint32_t lane) { return (2ull << lane) - 1; }     // the bits of lanes 0 .. lane

// the fold of a workgroup's values (commutative folds: a butterfly, every lane ends with the same bits)
template <typename OP>
__device__ __forceinline__ typename OP::S grp_block_fold(typename OP::S v, typename OP::S *lds, uint32_t tid) {
    using S = typename OP::S;
    for (int o = 32; o >= 1; o >>= 1) v = OP::combine(v, grp_shfl_xor(v, o));
    __syncthreads();                                    // lds may still be read from an earlier fold
    if ((tid & 63) == 0) lds[tid >> 6] = v;
    __syncthreads();
    S t = lds[0];
#pragma unroll
    for (int w = 1; w < GRP_WAVES; w++) t = OP::combine(t, lds[w]);
    return t;
}

// One tile of the segmented scan.  e[k]: in, the lane's element of load k; out, the fold from the nearest head at or before
// the lane's position (through the carry where the tile holds none before it).  H[k]: the load's head word (all zero: an
// ordinary scan).  carry: the fold of the cells since the last head before the tile; leaves as the same for the next tile.
// s_v / s_f: this tile's LDS buffer (the caller alternates two, so one barrier per tile is enough).
template <typename OP>
__device__ __forceinline__ void grp_tile_scan(typename OP::S (&e)[GRP_LOADS], const uint64_t (&H)[GRP_LOADS], typename OP::S &carry,
                                              typename OP::S *s_v, uint32_t *s_f, uint32_t wave, uint32_t lane) {
    using S = typename OP::S;
    uint32_t seg[GRP_LOADS];                            // the lane of the nearest head at or below this one, 0 when there is none
#pragma unroll
    for (int k = 0; k < GRP_LOADS; k++) {
        const uint64_t m = H[k] & grp_upto(lane);
        seg[k] = m ? 63u - (uint32_t)__clzll((long long)m) : 0u;
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
#pragma unroll
        for (int k = 0; k < GRP_LOADS; k++) {           // GRP_LOADS independent chains
            const S u = cum_shfl_up(e[k], s);
            if (lane >= seg[k] + (uint32_t)s) e[k] = OP::combine(u, e[k]);     // no head in (lane - s, lane]
        }
    }
    // ---- the loads chained through their lane-63 totals; the waves through LDS ----
    S before[GRP_LOADS];                                // the wave's cells in front of load k, from its last head when it has one
    bool cut[GRP_LOADS];
    S run = OP::identity();
    bool runf = false;
#pragma unroll
    for (int k = 0; k < GRP_LOADS; k++) {
        before[k] = run; cut[k] = runf;
        const S tot = cum_shfl(e[k], 63);
        if (H[k]) { run = tot; runf = true; }           // (uniform)
        else run = OP::combine(run, tot);
    }
    if (lane == 0) { s_v[wave] = run; s_f[wave] = runf; }
    __syncthreads();                                    // the one barrier of the tile
    S wpre = carry, total = carry;
#pragma unroll
    for (int w = 0; w < GRP_WAVES; w++) {
        const S x = s_v[w];
        const bool f = s_f[w] != 0;
        total = f ? x : OP::combine(total, x);
        if ((uint32_t)w < wave) wpre = f ? x : OP::combine(wpre, x);
    }
    carry = total;
#pragma unroll
    for (int k = 0; k < GRP_LOADS; k++) {
        if (H[k] & grp_upto(lane)) continue;            // a head at or below the lane in its own load: e[k] is complete
        e[k] = OP::combine(cut[k] ? before[k] : OP::combine(wpre, before[k]), e[k]);
    }
}

// the 64-bit word of the 64 positions from p (a multiple of 64), wave-uniform
__device__ __forceinline__ uint64_t grp_word(const uint64_t *words, int64_t p) { return words[p >> 6]; }

// ---- group heads -------------------------------------------------------------------------------------------------------------
// offsets[] ascends, so the heads that fall into one 32-bit word sit in consecutive lanes: the run ORs its bits together by
// cross-lane moves and its last lane issues the one atomic (all singletons: 32 heads per word, same-address atomics serialise)
__global__ __launch_bounds__(256) void grp_heads_kernel(const int64_t *offsets, int64_t n_groups, uint32_t *words) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    const int64_t p = g < n_groups ? offsets[g] : -1;   // (no early return: every lane takes part in the moves)
    const long long w = p >> 5;                         // -1: no head in this lane
    uint32_t bit = p >= 0 ? 1u << (p & 31) : 0u;
    for (int s = 1; s < 32; s <<= 1) {                  // a run is at most 32 lanes long
        const uint32_t ub = (uint32_t)__shfl_up((int)bit, s, 64);
        const long long uw = __shfl_up(w, s, 64);
        if (lane >= (uint32_t)s && uw == w) bit |= ub;
    }
    const long long next = __shfl_down(w, 1, 64);
    if (p >= 0 && (lane == 63 || next != w)) atomicOr(&words[w], bit);
}

// ---- the gather: one tile's cells through rows[], left contiguous with their null bits as ballot words ------------------------
__device__ __forceinline__ void grp_gather_tile(const CumCol &c, const GrpIn &g, int64_t p0, uint32_t wave, uint32_t lane,
                                                uint64_t (&x)[GRP_LOADS], bool (&nul)[GRP_LOADS]) {
    int64_t r[GRP_LOADS];
#pragma unroll
    for (int k = 0; k < GRP_LOADS; k++) {               // every load is issued before the first is used
        const int64_t j = p0 + wave * GRP_WAVE_ROWS + k * 64 + lane;
        r[k] = j < g.n ? g.rows[j] : -1;
    }
#pragma unroll
    for (int k = 0; k < GRP_LOADS; k++) {
        x[k] = r[k] >= 0 ? c.data[r[k]] : 0;
        nul[k] = r[k] >= 0 && c.mask && bit_at(c.mask, r[k]);
    }
#pragma unroll
    for (int k = 0; k < GRP_LOADS; k++) {
        const int64_t l0 = p0 + wave * GRP_WAVE_ROWS + k * 64;
        const uint64_t nb = __ballot(nul[k]);
        if (r[k] >= 0) g.cells[l0 + lane] = x[k];
        if (lane == 0) g.nullw[l0 >> 6] = nb;
    }
}

// lag: nothing to fold, the gather alone
__global__ __launch_bounds__(GRP_THREADS) void grp_gather_kernel(CumCol c, GrpIn g, int64_t tiles) {
    const uint32_t tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        uint64_t x[GRP_LOADS];
        bool nul[GRP_LOADS];
        grp_gather_tile(c, g, t * GRP_TILE, wave, lane, x, nul);
    }
}

// ---- the folds: reduce, then apply ------------------------------------------------------------------------------------------------
template <typename OP, bool IS_I64>
__global__ __launch_bounds__(GRP_THREADS) void grp_reduce_kernel(CumCol c, GrpIn g, GrpSpans sp) {
    using S = typename OP::S;
    __shared__ S s_v[2][GRP_WAVES];
    __shared__ uint32_t s_f[2][GRP_WAVES];
    const uint32_t tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int64_t b = blockIdx.x;
    const int64_t t0 = b * sp.base + (b < sp.rem ? b : sp.rem), t1 = t0 + sp.base + (b < sp.rem ? 1 : 0);
    S carry = OP::identity();
    bool seen = false;                                  // the span holds a head so far
    int buf = 0;
    for (int64_t t = t0; t < t1; t++, buf ^= 1) {
        const int64_t p0 = t * GRP_TILE;
        uint64_t x[GRP_LOADS];
        bool nul[GRP_LOADS];
        grp_gather_tile(c, g, p0, wave, lane, x, nul);
        S acc = OP::identity();                         // the wave's cells after its last head: the folds commute, so per lane first
        bool wf = false;
#pragma unroll
        for (int k = 0; k < GRP_LOADS; k++) {
            const int64_t l0 = p0 + wave * GRP_WAVE_ROWS + k * 64;
            const uint64_t H = grp_word(g.heads, l0);
            const S el = OP::elem(cum_f64(x[k], IS_I64), nul[k] || l0 + lane >= g.n);
            if (H) {                                    // (uniform) everything before the load's last head is cut off
                acc = lane >= 63u - (uint32_t)__clzll((long long)H) ? el : OP::identity();
                wf = true;
            } else {
                acc = OP::combine(acc, el);
            }
        }
        for (int o = 32; o >= 1; o >>= 1) acc = OP::combine(acc, grp_shfl_xor(acc, o));
        if (lane == 0) { s_v[buf][wave] = acc; s_f[buf][wave] = wf; }
        __syncthreads();                                // the one barrier of the tile: the other buffer is free by the next
#pragma unroll
        for (int w = 0; w < GRP_WAVES; w++) {
            const S v = s_v[buf][w];
            if (s_f[buf][w]) { carry = v; seen = true; }
            else carry = OP::combine(carry, v);
        }
    }
    if (tid == 0) {
        static_cast<S *>(sp.sum_v)[b] = carry;
        sp.sum_f[b] = seen;
    }
}

template <typename OP, bool IS_I64>
__global__ __launch_bounds__(GRP_THREADS) void grp_apply_kernel(GrpIn g, GrpSpans sp, CumOut o) {
    using S = typename OP::S;
    constexpr bool IS_COUNT = OP::IS_COUNT;
    __shared__ S s_fold[GRP_WAVES];
    __shared__ uint32_t s_from[GRP_WAVES];
    __shared__ S s_v[2][GRP_WAVES];
    __shared__ uint32_t s_f[2][GRP_WAVES];
    const uint32_t tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int64_t b = blockIdx.x;
    const int64_t t0 = b * sp.base + (b < sp.rem ? b : sp.rem), t1 = t0 + sp.base + (b < sp.rem ? 1 : 0);
    if (t0 >= t1) return;                               // (uniform: an empty span)

    // ---- the carry: the summaries of the earlier spans, back to the nearest one that holds a head ----
    uint32_t from = 0;                                  // (span 0 starts at position 0, a head)
    for (int64_t j = tid; j < b; j += GRP_THREADS)
        if (sp.sum_f[j]) from = (uint32_t)j;            // ascending j: the thread's last
    from = grp_block_fold<GrpStart>(from, s_from, tid);
    S carry = OP::identity();
    for (int64_t j = (int64_t)from + tid; j < b; j += GRP_THREADS) carry = OP::combine(carry, static_cast<const S *>(sp.sum_v)[j]);
    carry = grp_block_fold<OP>(carry, s_fold, tid);

    uint32_t nulls = 0;
    int buf = 0;
    for (int64_t t = t0; t < t1; t++, buf ^= 1) {
        const int64_t p0 = t * GRP_TILE;
        int64_t r[GRP_LOADS];
        uint64_t x[GRP_LOADS], H[GRP_LOADS], nw[GRP_LOADS];
#pragma unroll
        for (int k = 0; k < GRP_LOADS; k++) {           // every load is issued before the first is used
            const int64_t l0 = p0 + wave * GRP_WAVE_ROWS + k * 64, j = l0 + lane;
            r[k] = j < g.n ? g.rows[j] : -1;
            x[k] = j < g.n ? g.cells[j] : 0;
            H[k] = grp_word(g.heads, l0);
            nw[k] = grp_word(g.nullw, l0);
        }
        S e[GRP_LOADS];
#pragma unroll
        for (int k = 0; k < GRP_LOADS; k++) e[k] = OP::elem(cum_f64(x[k], IS_I64), ((nw[k] >> lane) & 1) || r[k] < 0);
        grp_tile_scan<OP>(e, H, carry, s_v[buf], s_f[buf], wave, lane);
#pragma unroll
        for (int k = 0; k < GRP_LOADS; k++) {
            uint64_t v = OP::out(OP::combine(OP::start(), e[k]));
            if (!IS_COUNT && ((nw[k] >> lane) & 1)) v = CANON_NAN;         // a null row is NaN under its bit; the running count is written as it is
            if (r[k] >= 0) o.data[r[k]] = v;
            if (!IS_COUNT && lane == 0) nulls += __popcll(nw[k]);
        }
    }
    if (lane == 0 && nulls) atomicAdd(o.n_null, nulls);
}

// ---- the first position of every position's group: an ordinary max-scan of the head positions ---------------------------------------
__global__ __launch_bounds__(GRP_THREADS) void grp_start_reduce_kernel(GrpIn g, GrpSpans sp) {
    __shared__ uint32_t s_fold[GRP_WAVES];
    const uint32_t tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t t0 = b * sp.base + (b < sp.rem ? b : sp.rem), t1 = t0 + sp.base + (b < sp.rem ? 1 : 0);
    uint32_t last = 0;                                  // the span's last head position
    for (int64_t w = t0 * (GRP_TILE / 64) + tid; w < t1 * (GRP_TILE / 64); w += GRP_THREADS) {     // ascending words: the thread's last
        const uint64_t H = g.heads[w];
        if (H) last = (uint32_t)(w * 64 + 63 - __clzll((long long)H));
    }
    last = grp_block_fold<GrpStart>(last, s_fold, tid);
    if (tid == 0) static_cast<uint32_t *>(sp.sum_v)[b] = last;
}

__global__ __launch_bounds__(GRP_THREADS) void grp_start_apply_kernel(GrpIn g, GrpSpans sp) {
    __shared__ uint32_t s_fold[GRP_WAVES];
    __shared__ uint32_t s_v[2][GRP_WAVES];
    __shared__ uint32_t s_f[2][GRP_WAVES];
    const uint32_t tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int64_t b = blockIdx.x;
    const int64_t t0 = b * sp.base + (b < sp.rem ? b : sp.rem), t1 = t0 + sp.base + (b < sp.rem ? 1 : 0);
    if (t0 >= t1) return;                               // (uniform: an empty span)
    uint32_t carry = 0;
    for (int64_t j = tid; j < b; j += GRP_THREADS) carry = GrpStart::combine(carry, static_cast<const uint32_t *>(sp.sum_v)[j]);
    carry = grp_block_fold<GrpStart>(carry, s_fold, tid);
    int buf = 0;
    for (int64_t t = t0; t < t1; t++, buf ^= 1) {
        const int64_t p0 = t * GRP_TILE;
        uint32_t e[GRP_LOADS];
        uint64_t none[GRP_LOADS];
#pragma unroll
        for (int k = 0; k < GRP_LOADS; k++) {
            const int64_t l0 = p0 + wave * GRP_WAVE_ROWS + k * 64;
            e[k] = ((grp_word(g.heads, l0) >> lane) & 1) ? (uint32_t)(l0 + lane) : 0u;
            none[k] = 0;
        }
        grp_tile_scan<GrpStart>(e, none, carry, s_v[buf], s_f[buf], wave, lane);
#pragma unroll
        for (int k = 0; k < GRP_LOADS; k++) {
            const int64_t j = p0 + wave * GRP_WAVE_ROWS + k * 64 + lane;
            if (j < g.n) g.start[j] = e[k];
        }
    }
}

// ---- lag and the row number: one stream over the positions ------------------------------------------------------------------------
__device__ __forceinline__ bool grp_null_at(const GrpIn &g, int64_t j) { return (g.nullw[j >> 6] >> (j & 63)) & 1; }

// bitmap: the output null bits by ROW as zeroed 32-bit words, or nullptr (the count alone)
template <int OP, bool IS_I64>
__global__ __launch_bounds__(GRP_THREADS) void grp_lag_kernel(GrpIn g, int64_t tiles, int64_t periods, CumOut o, uint32_t *bitmap) {
    const uint32_t lane = threadIdx.x & 63;
    uint32_t nulls = 0;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
#pragma unroll
        for (int k = 0; k < GRP_TILE / GRP_THREADS; k++) {
            const int64_t j = t * GRP_TILE + k * GRP_THREADS + threadIdx.x;
            if (j >= g.n) continue;
            const int64_t r = g.rows[j];
            const uint32_t st = g.start[j];
            if (OP == PANDRS_HIP_GROUPED_ROW_NUMBER) {
                o.data[r] = (uint64_t)(j - (int64_t)st);
                continue;
            }
            const int64_t s = j - periods;
            const bool has = s >= 0 && s < g.n && g.start[s] == st;        // the source sits in the same group
            uint64_t v = CANON_NAN;
            bool gone = false;
            if (OP == PANDRS_HIP_GROUPED_SHIFT) {
                if (!has || grp_null_at(g, s)) gone = true;
                else v = cum_bits(cum_f64(g.cells[s], IS_I64));
            } else if (has) {                           // no source: the reference's vec![NAN; n], a value, not a missing row
                if (grp_null_at(g, j) || grp_null_at(g, s)) {
                    gone = true;
                } else {
                    const double curr = cum_f64(g.cells[j], IS_I64), prev = cum_f64(g.cells[s], IS_I64);
                    if (OP == PANDRS_HIP_GROUPED_DIFF) v = cum_bits(curr - prev);
                    else v = prev == 0.0 ? CANON_NAN : cum_bits((curr - prev) / prev);
                }
            }
            o.data[r] = v;
            if (gone) {
                nulls++;
                if (bitmap) atomicOr(&bitmap[r >> 5], 1u << (r & 31));
            }
        }
    }
    if (OP == PANDRS_HIP_GROUPED_ROW_NUMBER) return;
    for (int s = 32; s >= 1; s >>= 1) nulls += __shfl_down((int)nulls, s, 64);
    if (lane == 0 && nulls) atomicAdd(o.n_null, nulls);
}

// the output mask, stored bytewise: a copy of `src` (the column's own mask, or the lag bitmap) with the bits past n cleared
__global__ __launch_bounds__(256) void grp_mask_store_kernel(const uint8_t *src, uint8_t *dst, int64_t n) {
    const int64_t byte = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, left = n - byte * 8;
    if (left > 0) dst[byte] = src[byte] & (left >= 8 ? 0xFFu : (0xFFu >> (8 - left)));
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
template <typename OP>
static void grp_fold_launch(pandrs_hip_ctx *c, int grid, bool is_i64, const CumCol &cc, const GrpIn &g, const GrpSpans &sp, const CumOut &co) {
    if (is_i64) {
        hipLaunchKernelGGL((grp_reduce_kernel<OP, true>), dim3(grid), dim3(GRP_THREADS), 0, c->stream, cc, g, sp);
        hipLaunchKernelGGL((grp_apply_kernel<OP, true>), dim3(grid), dim3(GRP_THREADS), 0, c->stream, g, sp, co);
    } else {
        hipLaunchKernelGGL((grp_reduce_kernel<OP, false>), dim3(grid), dim3(GRP_THREADS), 0, c->stream, cc, g, sp);
        hipLaunchKernelGGL((grp_apply_kernel<OP, false>), dim3(grid), dim3(GRP_THREADS), 0, c->stream, g, sp, co);
    }
}

template <int OP>
static void grp_lag_launch(pandrs_hip_ctx *c, int grid, bool is_i64, const GrpIn &g, int64_t tiles, int64_t periods, const CumOut &co, uint32_t *bitmap) {
    if (is_i64) hipLaunchKernelGGL((grp_lag_kernel<OP, true>), dim3(grid), dim3(GRP_THREADS), 0, c->stream, g, tiles, periods, co, bitmap);
    else hipLaunchKernelGGL((grp_lag_kernel<OP, false>), dim3(grid), dim3(GRP_THREADS), 0, c->stream, g, tiles, periods, co, bitmap);
}

int32_t grouped_entry(pandrs_hip_ctx *c, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows, int32_t op, int64_t periods,
                      int32_t out_mem_space, void *out_data, uint8_t *out_null_mask, int64_t *out_n_null) {
    const bool numbers = op == PANDRS_HIP_GROUPED_ROW_NUMBER;       // reads no column
    if (!c || n_rows < 0 || (!numbers && !col) || (n_rows > 0 && (!out_data || (!numbers && !col->data))))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "grouped: bad arguments");
    ST_TRY(check_mem_space("grouped", mem_space, out_mem_space));
    if (op < PANDRS_HIP_GROUPED_CUM_SUM || op > PANDRS_HIP_GROUPED_PCT_CHANGE)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "grouped: op %d is not a pandrs_hip_grouped_op", op);
    const bool lag = op >= PANDRS_HIP_GROUPED_SHIFT;
    if (lag && op != PANDRS_HIP_GROUPED_SHIFT && periods < 0)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "grouped: periods %lld is negative; only SHIFT looks ahead", (long long)periods);
    {
        std::lock_guard<std::mutex> lock(c->mu);
        if (!c->gr.valid)
            return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "grouped: no grouping retained in this context; call pandrs_hip_groupby_indices first");
        if (c->gr.n_rows != n_rows)
            return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "grouped: n_rows is %lld, the retained grouping has %lld rows", (long long)n_rows,
                        (long long)c->gr.n_rows);
    }
    const pandrs_hip_column none{nullptr, nullptr, PANDRS_HIP_I64};
    if (numbers) col = &none;
    const bool is_i64 = col->dtype == PANDRS_HIP_I64;
    periods = std::max<int64_t>(-n_rows, std::min<int64_t>(n_rows, periods));      // past either end no row has a source
    return cum_call("grouped", c, mem_space, col, n_rows, out_mem_space, out_data, out_null_mask, out_n_null, [&](const CumCol &cc, CumOut &co) -> int32_t {
        // ---- the counter, the head and null words, the gathered cells, the starts, the lag bitmap and the span summaries in one
        //      arena, sized up front; the grouping itself lives in c->groups and is only read ----
        const GroupsResult &gr = c->gr;
        const int64_t tiles = (n_rows + GRP_TILE - 1) / GRP_TILE, nbytes = (n_rows + 7) / 8;
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)c->n_cu * GRP_BLOCKS_PER_CU, tiles));
        const size_t words = (size_t)tiles * (GRP_TILE / 64), n = (size_t)n_rows, max_grid = (size_t)c->n_cu * GRP_BLOCKS_PER_CU;
        const bool starts = lag || numbers, want_bitmap = lag && co.mask;
        ST_TRY(c->work.ensure(Arena::padded(4) + 2 * Arena::padded(words * 8) + (numbers ? 0 : Arena::padded(n * 8)) +
                              (starts ? Arena::padded(n * 4) : 0) + (want_bitmap ? Arena::padded((n + 31) / 32 * 4) : 0) +
                              Arena::padded(max_grid * 8) + Arena::padded(max_grid * 4), c->stream));
        co.n_null = c->work.take<uint32_t>(1);
        uint64_t *heads = c->work.take<uint64_t>(words);
        GrpIn g{gr.rows, heads, nullptr, c->work.take<uint64_t>(words), nullptr, n_rows};
        if (!numbers) g.cells = c->work.take<uint64_t>(n);
        if (starts) g.start = c->work.take<uint32_t>(n);
        uint32_t *bitmap = want_bitmap ? c->work.take<uint32_t>((n + 31) / 32) : nullptr;
        GrpSpans sp{tiles, tiles / grid, tiles % grid, c->work.take<uint64_t>(max_grid), c->work.take<uint32_t>(max_grid)};
        if (!co.n_null || !heads || !g.nullw || (!numbers && !g.cells) || (starts && !g.start) || (want_bitmap && !bitmap) || !sp.sum_v || !sp.sum_f)
            return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (grouped)");
        HIP_TRY(hipMemsetAsync(co.n_null, 0, 4, c->stream));
        HIP_TRY(hipMemsetAsync(heads, 0, words * 8, c->stream));
        if (bitmap) HIP_TRY(hipMemsetAsync(bitmap, 0, (n + 31) / 32 * 4, c->stream));
        hipLaunchKernelGGL(grp_heads_kernel, dim3((unsigned)((gr.n_groups + 255) / 256)), dim3(256), 0, c->stream, gr.offsets, gr.n_groups,
                           reinterpret_cast<uint32_t *>(heads));
        const dim3 mask_grid((unsigned)((nbytes + 255) / 256));
        if (starts) {
            hipLaunchKernelGGL(grp_start_reduce_kernel, dim3(grid), dim3(GRP_THREADS), 0, c->stream, g, sp);
            hipLaunchKernelGGL(grp_start_apply_kernel, dim3(grid), dim3(GRP_THREADS), 0, c->stream, g, sp);
            if (lag) hipLaunchKernelGGL(grp_gather_kernel, dim3(grid), dim3(GRP_THREADS), 0, c->stream, cc, g, tiles);
            switch (op) {
            case PANDRS_HIP_GROUPED_ROW_NUMBER: grp_lag_launch<PANDRS_HIP_GROUPED_ROW_NUMBER>(c, grid, is_i64, g, tiles, 0, co, nullptr); break;
            case PANDRS_HIP_GROUPED_SHIFT: grp_lag_launch<PANDRS_HIP_GROUPED_SHIFT>(c, grid, is_i64, g, tiles, periods, co, bitmap); break;
            case PANDRS_HIP_GROUPED_DIFF: grp_lag_launch<PANDRS_HIP_GROUPED_DIFF>(c, grid, is_i64, g, tiles, periods, co, bitmap); break;
            default: grp_lag_launch<PANDRS_HIP_GROUPED_PCT_CHANGE>(c, grid, is_i64, g, tiles, periods, co, bitmap); break;
            }
            if (bitmap) hipLaunchKernelGGL(grp_mask_store_kernel, mask_grid, dim3(256), 0, c->stream, reinterpret_cast<const uint8_t *>(bitmap), co.mask, n_rows);
        } else {
            switch (op) {
            case PANDRS_HIP_GROUPED_CUM_SUM: grp_fold_launch<CumSum>(c, grid, is_i64, cc, g, sp, co); break;
            case PANDRS_HIP_GROUPED_CUM_MAX: grp_fold_launch<CumExt<true>>(c, grid, is_i64, cc, g, sp, co); break;
            case PANDRS_HIP_GROUPED_CUM_MIN: grp_fold_launch<CumExt<false>>(c, grid, is_i64, cc, g, sp, co); break;
            default: grp_fold_launch<CumCount>(c, grid, is_i64, cc, g, sp, co); break;
            }
            // a fold's output mask is the input's, bits past n_rows cleared: a copy, no scatter
            if (co.mask && cc.mask && op != PANDRS_HIP_GROUPED_CUM_COUNT)
                hipLaunchKernelGGL(grp_mask_store_kernel, mask_grid, dim3(256), 0, c->stream, cc.mask, co.mask, n_rows);
        }
        if (co.mask && (numbers || op == PANDRS_HIP_GROUPED_CUM_COUNT || (!lag && !cc.mask))) HIP_TRY(hipMemsetAsync(co.mask, 0, (size_t)nbytes, c->stream));
        // the streams run: offsets once; rows[] once per pass that gathers or scatters; the column, the gathered cells (written, read)
        // and the output; the starts written and read; the masks
        int64_t bytes = gr.n_groups * 8 + (int64_t)words * 8;
        if (numbers) bytes += n_rows * (4 + 4 + 8 + 8);
        else if (lag) bytes += n_rows * (8 + 8 + 8 + 4 + 8 + 4 + 8 + 8) + (int64_t)words * 16;
        else bytes += n_rows * (8 + 8 + 8 + 8 + 8 + 8) + (int64_t)words * 16;
        c->timings.algorithmic_bytes = bytes + (cc.mask ? nbytes : 0) + (co.mask ? nbytes : 0);
        return 0;
    });
}

}  // namespace pandrs
