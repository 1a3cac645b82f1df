// sort.hip — the stable multi-key row order behind OptimizedDataFrame::sort_by / sort_by_columns
// (reference src/optimized/split_dataframe/sort.rs:18-272), gfx950, wave64.
//
// 1. Encode.  Every key column becomes an order-preserving unsigned code of just the bits it uses
//    (a min / max pass first): value code = sortable(x) - min ascending, max - sortable(x) descending;
//    NaN = span + 1, null = span + 1 + has_nan, so NaN and null sort last in BOTH directions.  The codes
//    are concatenated MSB-first (key 0 most significant) into W = ceil(bits / 64) words per row.
// 2. LSD radix sort over the bits that vary (an AND / OR pass per word trims constant bits at both ends),
//    least significant word first, digits of <= SORT_MAX_DIGIT bits.  Every pass is reduce-then-scan:
//    a digit histogram per workgroup's row range, one exclusive scan of the digit-major counts, and a
//    stable scatter in which each workgroup walks its range tile by tile, ranks the rows of a tile with
//    wave ballots (equal digits keep row order) and stages them in LDS so the writes are coalesced.
//    No inter-workgroup spinning: every hand-off between workgroups is a kernel boundary.
// 3. Words above the first are re-gathered by row at the start of their passes (only keys wider than
//    64 bits in total pay it).  The last pass writes the int64 row indices the gathers take.
#include "engine.hpp"

#include <algorithm>
#include <vector>

namespace pandrs {

constexpr int SORT_THREADS = 256;                       // 4 waves
constexpr int SORT_WAVES = SORT_THREADS / 64;
constexpr int SORT_RPL = 8;                             // rows per lane in a tile
constexpr int SORT_TILE = SORT_THREADS * SORT_RPL;      // 2048 rows
constexpr int SORT_HIST_THREADS = 1024;                 // the histogram: 16 waves per workgroup keep more loads in flight
constexpr int SORT_MAX_DIGIT = 8;
constexpr int SORT_MAX_BUCKETS = 1 << SORT_MAX_DIGIT;
constexpr int SORT_BLOCKS_PER_CU = 4;                   // the scatter takes 26 KB of LDS: four workgroups per CU
static_assert(SORT_WAVES * SORT_MAX_BUCKETS * 4 <= SORT_TILE * 8, "the scatter's wave counters overlay its key staging");

// sortable image of one non-null, non-NaN cell: unsigned order == the reference's order
struct SortKeyDesc {
    KeyDesc key;
    const uint32_t *rank;   // U32CODE: rank[code] = position of the code's string in byte-wise order
    uint64_t n_codes;
};

__device__ __forceinline__ bool sort_is_nan(const SortKeyDesc &d, int64_t i) {
    if (d.key.dtype != PANDRS_HIP_F64) return false;
    const uint64_t b = reinterpret_cast<const uint64_t *>(d.key.data)[i];
    return (b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull;
}

__device__ __forceinline__ uint64_t sort_sortable(const SortKeyDesc &d, int64_t i) {
    switch (d.key.dtype) {
    case PANDRS_HIP_I64:
        return reinterpret_cast<const uint64_t *>(d.key.data)[i] ^ 0x8000000000000000ull;
    case PANDRS_HIP_F64: {
        uint64_t b = reinterpret_cast<const uint64_t *>(d.key.data)[i];
        if (b == 0x8000000000000000ull) b = 0;          // -0.0 == 0.0 (partial_cmp): they tie
        return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    }
    case PANDRS_HIP_U32CODE: {
        const uint32_t code = reinterpret_cast<const uint32_t *>(d.key.data)[i];
        return code < d.n_codes ? d.rank[code] : 0;     // (out-of-range codes were refused by the min / max pass)
    }
    default:
        return bit_at(reinterpret_cast<const uint8_t *>(d.key.data), i) ? 1ull : 0ull;
    }
}

// out[0] = min sortable, out[1] = max (non-null, non-NaN rows), out[2] |= 1 null seen, 2 NaN seen, 4 code >= n_codes
__global__ void sort_minmax_kernel(SortKeyDesc d, int64_t n, uint64_t *out) {
    uint64_t mn = ~0ull, mx = 0, fl = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (key_is_null(d.key, i)) { fl |= 1; continue; }
        if (sort_is_nan(d, i)) { fl |= 2; continue; }
        if (d.key.dtype == PANDRS_HIP_U32CODE && reinterpret_cast<const uint32_t *>(d.key.data)[i] >= d.n_codes) { fl |= 4; continue; }
        const uint64_t s = sort_sortable(d, i);
        mn = s < mn ? s : mn;
        mx = s > mx ? s : mx;
    }
    for (int o = 32; o >= 1; o >>= 1) {
        const uint64_t a = __shfl_down(mn, o, 64), b = __shfl_down(mx, o, 64), f = __shfl_down(fl, o, 64);
        mn = a < mn ? a : mn; mx = b > mx ? b : mx; fl |= f;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin((unsigned long long *)&out[0], mn);
        atomicMax((unsigned long long *)&out[1], mx);
        if (fl) atomicOr((unsigned long long *)&out[2], fl);
    }
}

struct SortEncode {
    SortKeyDesc d;
    uint64_t base;          // min (ascending) or max (descending) sortable value
    uint64_t span;          // max - min
    uint32_t asc, has_nan;
    uint32_t off;           // bit position of the code's LSB in the concatenated key
    uint32_t width;         // bits of the code (<= 66)
    uint32_t fresh;         // bit t: word off / 64 + t is written (not OR-ed) by this key
    int64_t n;
    uint64_t *words;        // [W][stride]
    size_t stride;
    uint32_t W;
};

// the key's code (<= 66 bits) OR-ed into the words it touches
__global__ void sort_encode_kernel(SortEncode e) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= e.n) return;
    unsigned __int128 code;
    if (key_is_null(e.d.key, i)) code = (unsigned __int128)e.span + 1 + e.has_nan;
    else if (sort_is_nan(e.d, i)) code = (unsigned __int128)e.span + 1;
    else {
        const uint64_t s = sort_sortable(e.d, i);
        code = e.asc ? s - e.base : e.base - s;
    }
    const uint32_t j0 = e.off >> 6, sh = e.off & 63, nw = (sh + e.width + 63) >> 6;   // nw <= 3 words
    for (uint32_t t = 0; t < nw; t++) {
        const uint64_t part = t == 0 ? (uint64_t)(code << sh) : (uint64_t)(code >> (64 * t - sh));   // (64 t - sh < 128: t = 2 needs sh > 62)
        uint64_t *w = e.words + (size_t)(j0 + t) * e.stride + i;
        if ((e.fresh >> t) & 1) *w = part;
        else if (part) *w |= part;
    }
}

// out[2j] = AND of word j over all rows, out[2j+1] = OR: bits with AND == OR never vary
__global__ void sort_word_andor_kernel(const uint64_t *words, size_t stride, uint32_t W, int64_t n, uint64_t *out) {
    for (uint32_t j = 0; j < W; j++) {
        uint64_t a = ~0ull, o = 0;
        const uint64_t *w = words + (size_t)j * stride;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
            a &= w[i]; o |= w[i];
        }
        for (int s = 32; s >= 1; s >>= 1) { a &= __shfl_down(a, s, 64); o |= __shfl_down(o, s, 64); }
        if ((threadIdx.x & 63) == 0) {
            atomicAnd((unsigned long long *)&out[2 * j], a);
            atomicOr((unsigned long long *)&out[2 * j + 1], o);
        }
    }
}

// cur[i] = word[row[i]]: the next word of a wide key in the order the previous passes left
__global__ void sort_regather_kernel(const uint64_t *word, const uint32_t *rows, int64_t n, uint64_t *cur) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) cur[i] = word[rows[i]];
}

__global__ void sort_iota_kernel(int64_t n, int64_t *out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = i;
}

// lanes of the wave holding the same digit as this lane (among `valid` lanes)
__device__ __forceinline__ uint64_t sort_peers(uint32_t dg, int dbits, uint64_t valid) {
    uint64_t peers = valid;
    for (int b = 0; b < dbits; b++) {
        const uint64_t bal = __ballot((dg >> b) & 1);
        peers &= ((dg >> b) & 1) ? bal : ~bal;
    }
    return peers;
}

__device__ __forceinline__ uint64_t lanes_below() {
    const uint32_t lane = threadIdx.x & 63;
    return lane == 0 ? 0ull : (~0ull >> (64 - lane));
}

struct SortPass {
    const uint64_t *kin;
    uint64_t *kout;          // nullptr on the last pass: keys are not needed afterwards
    const uint32_t *rin;     // nullptr on the first pass: the row is the position
    uint32_t *rout;          // u32 rows (not the last pass)
    int64_t *rout64;         // int64 rows (the last pass)
    uint32_t *counts;        // [buckets][G]
    const uint32_t *offs;    // exclusive scan of counts
    int64_t n, rows_per_block;
    uint32_t G, shift, dbits;
};

// counts[d * G + b] = rows of block b's range whose digit is d
__global__ __launch_bounds__(SORT_HIST_THREADS) void sort_hist_kernel(SortPass p) {
    __shared__ uint32_t h[SORT_MAX_BUCKETS];
    const uint32_t nb = 1u << p.dbits, mask = nb - 1;
    for (uint32_t d = threadIdx.x; d < nb; d += SORT_HIST_THREADS) h[d] = 0;
    __syncthreads();
    const int64_t beg = (int64_t)blockIdx.x * p.rows_per_block, end = min(p.n, beg + p.rows_per_block);
    const uint64_t below = lanes_below();
    // (64 consecutive rows per wave step; a uniform loop so that the ballots see every lane)
    for (int64_t c = beg + (int64_t)(threadIdx.x >> 6) * 64; c < end; c += SORT_HIST_THREADS) {
        const int64_t i = c + (threadIdx.x & 63);
        const bool ok = i < end;
        const uint32_t dg = ok ? (uint32_t)(p.kin[i] >> p.shift) & mask : 0;
        const uint64_t peers = sort_peers(dg, p.dbits, __ballot(ok));
        if (ok && !(peers & below)) atomicAdd(&h[dg], (uint32_t)__popcll(peers));
    }
    __syncthreads();
    for (uint32_t d = threadIdx.x; d < nb; d += SORT_HIST_THREADS) p.counts[(size_t)d * p.G + blockIdx.x] = h[d];
}

// Block b scatters its row range tile by tile, in row order; within a tile, wave w owns rows
// [w * 64 * SORT_RPL, (w + 1) * 64 * SORT_RPL) and ranks them 64 at a time, so a row's rank counts exactly the
// rows before it (in row order) with the same digit.
template <bool LAST>
__global__ __launch_bounds__(SORT_THREADS) void sort_scatter_kernel(SortPass p) {
    __shared__ __attribute__((aligned(16))) uint64_t stage_k[SORT_TILE];   // overlays wave_hist
    __shared__ uint32_t stage_r[SORT_TILE];
    __shared__ uint32_t lstart[SORT_MAX_BUCKETS + 1];                      // tile-local exclusive scan over digits
    __shared__ uint32_t goff[SORT_MAX_BUCKETS];                            // running global offset per digit
    __shared__ uint32_t wsum[SORT_WAVES];
    uint32_t *wave_hist = reinterpret_cast<uint32_t *>(stage_k);           // [SORT_WAVES][SORT_MAX_BUCKETS]
    const uint32_t nb = 1u << p.dbits, mask = nb - 1;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint64_t below = lanes_below();
    for (uint32_t d = tid; d < nb; d += SORT_THREADS) goff[d] = p.offs[(size_t)d * p.G + blockIdx.x];
    const int64_t beg = (int64_t)blockIdx.x * p.rows_per_block, end = min(p.n, beg + p.rows_per_block);
    for (int64_t t0 = beg; t0 < end; t0 += SORT_TILE) {
        const uint32_t rows = (uint32_t)min((int64_t)SORT_TILE, end - t0);
        __syncthreads();                                   // the previous tile's staging and goff are consumed
        for (uint32_t d = lane; d < nb; d += 64) wave_hist[wave * SORT_MAX_BUCKETS + d] = 0;
        // (wave-private counters: the wave's own LDS ops are in order, no barrier needed)
        uint64_t key[SORT_RPL];
        uint32_t row[SORT_RPL], dig[SORT_RPL], rank[SORT_RPL];
#pragma unroll
        for (int r = 0; r < SORT_RPL; r++) {
            const uint32_t li = wave * (SORT_RPL * 64) + r * 64 + lane;
            const bool ok = li < rows;
            const int64_t i = t0 + li;
            key[r] = ok ? p.kin[i] : 0;
            row[r] = ok ? (p.rin ? p.rin[i] : (uint32_t)i) : 0;
        }
#pragma unroll
        for (int r = 0; r < SORT_RPL; r++) {
            const uint32_t li = wave * (SORT_RPL * 64) + r * 64 + lane;
            const bool ok = li < rows;
            const uint32_t dg = (uint32_t)(key[r] >> p.shift) & mask;
            const uint64_t peers = sort_peers(dg, p.dbits, __ballot(ok));
            uint32_t base = ok ? wave_hist[wave * SORT_MAX_BUCKETS + dg] : 0;
            if (ok && !(peers & below)) wave_hist[wave * SORT_MAX_BUCKETS + dg] = base + (uint32_t)__popcll(peers);
            dig[r] = dg;
            rank[r] = base + (uint32_t)__popcll(peers & below);
        }
        __syncthreads();
        // per digit: exclusive prefix over the waves (in place) and the tile's count
        for (uint32_t d = tid; d < nb; d += SORT_THREADS) {
            uint32_t run = 0;
            for (int w = 0; w < SORT_WAVES; w++) {
                const uint32_t v = wave_hist[w * SORT_MAX_BUCKETS + d];
                wave_hist[w * SORT_MAX_BUCKETS + d] = run;
                run += v;
            }
            lstart[d] = run;
        }
        __syncthreads();
        {   // exclusive scan of lstart[0, nb): each thread owns ceil(nb / 256) consecutive digits
            const uint32_t per = (nb + SORT_THREADS - 1) / SORT_THREADS, d0 = tid * per;
            uint32_t s = 0;
            for (uint32_t k = 0; k < per && d0 + k < nb; k++) s += lstart[d0 + k];
            uint32_t inc = s;
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t v = __shfl_up(inc, o, 64);
                if (lane >= (uint32_t)o) inc += v;
            }
            if (lane == 63) wsum[wave] = inc;
            __syncthreads();
            uint32_t ex = inc - s;
            for (uint32_t w = 0; w < wave; w++) ex += wsum[w];
            for (uint32_t k = 0; k < per && d0 + k < nb; k++) {
                const uint32_t v = lstart[d0 + k];
                lstart[d0 + k] = ex;
                ex += v;
            }
            if (tid == 0) lstart[nb] = rows;
        }
        __syncthreads();
        uint32_t pos[SORT_RPL];
#pragma unroll
        for (int r = 0; r < SORT_RPL; r++)
            pos[r] = lstart[dig[r]] + wave_hist[wave * SORT_MAX_BUCKETS + dig[r]] + rank[r];
        __syncthreads();                                   // wave_hist is read: stage_k may overwrite it
#pragma unroll
        for (int r = 0; r < SORT_RPL; r++) {
            const uint32_t li = wave * (SORT_RPL * 64) + r * 64 + lane;
            if (li < rows) { stage_k[pos[r]] = key[r]; stage_r[pos[r]] = row[r]; }
        }
        __syncthreads();
        for (uint32_t j = tid; j < rows; j += SORT_THREADS) {
            const uint64_t k = stage_k[j];
            const uint32_t dg = (uint32_t)(k >> p.shift) & mask;
            const size_t dst = (size_t)goff[dg] + (j - lstart[dg]);
            if (dst >= (size_t)p.n) continue;              // (cannot happen with consistent counts; a guard, not a path)
            if (LAST) p.rout64[dst] = stage_r[j];
            else { p.rout[dst] = stage_r[j]; if (p.kout) p.kout[dst] = k; }
        }
        __syncthreads();
        for (uint32_t d = tid; d < nb; d += SORT_THREADS) goff[d] += lstart[d + 1] - lstart[d];
    }
}

// ------------------------------------------------------------------------------------------------------------------
struct SortDigit { uint32_t word, shift, dbits; };

// The stable order of n_rows (> 0) rows by keys the device can read, left on the device; the caller holds c->mu, has begun
// the timings and staged what was on the host.  d_out != nullptr: the permutation is written there (pandrs_hip_sort_indices).
// d_out == nullptr: *perm_out = n_rows int64 taken from c->work, which is then sized for the sort plus extra_work bytes: the
// caller takes its own buffers from c->work after the call (rank.hip).
static uint32_t sort_grid(const pandrs_hip_ctx *c, int64_t n_rows) {
    return (uint32_t)std::max<int64_t>(1, std::min<int64_t>((int64_t)c->n_cu * SORT_BLOCKS_PER_CU, (n_rows + SORT_TILE - 1) / SORT_TILE));
}

// codes [W][S] | second key buffer | two row buffers | counts | offsets | scan | and/or
size_t sort_order_workspace(const pandrs_hip_ctx *c, int64_t n_rows, uint32_t W) {
    const size_t n = (size_t)n_rows, n_counts = (size_t)SORT_MAX_BUCKETS * sort_grid(c, n_rows);
    const size_t S = (n + 31) & ~size_t(31);            // word stride in rows (whole 256-byte pieces)
    return Arena::padded((size_t)W * S * 8) + Arena::padded(n * 8) + 2 * Arena::padded(n * 4) + 2 * Arena::padded(n_counts * 4 + 4) +
           Arena::padded(scan_seg_count(n_counts) * 4) + Arena::padded((size_t)W * 16) + 4096;
}

int32_t sort_order_device(pandrs_hip_ctx *c, const KeyDesc *keys, int32_t n_keys, const int32_t *ascending, const uint32_t *d_rank,
                          int64_t n_codes, int64_t n_rows, int64_t *d_out, size_t extra_work, int64_t **perm_out) {
    const size_t n = (size_t)n_rows;
    const size_t own_work = (d_out ? 0 : Arena::padded(n * 8)) + extra_work;   // 0 for pandrs_hip_sort_indices
    std::vector<SortKeyDesc> kd(n_keys);
    for (int k = 0; k < n_keys; k++) {
        kd[k].key = keys[k];
        kd[k].rank = keys[k].dtype == PANDRS_HIP_U32CODE ? d_rank : nullptr;
        kd[k].n_codes = (uint64_t)n_codes;
    }

    // ---- code widths: one min / max pass per key, one read-back for all ----
    const int blocks_rd = (int)std::min<int64_t>(2048, (n_rows + 255) / 256);
    std::vector<uint64_t> mm(3 * (size_t)n_keys);
    {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_OTHER);
        ST_TRY(c->temp.ensure(Arena::padded(mm.size() * 8) + 4096, c->stream));
        uint64_t *d_mm = c->temp.take<uint64_t>(mm.size());
        if (!d_mm) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (sort)");
        for (int k = 0; k < n_keys; k++) { mm[3 * k] = ~0ull; mm[3 * k + 1] = 0; mm[3 * k + 2] = 0; }
        HIP_TRY(hipMemcpyAsync(d_mm, mm.data(), mm.size() * 8, hipMemcpyHostToDevice, c->stream));
        for (int k = 0; k < n_keys; k++)
            hipLaunchKernelGGL(sort_minmax_kernel, dim3(blocks_rd), dim3(256), 0, c->stream, kd[k], n_rows, d_mm + 3 * k);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(mm.data(), d_mm, mm.size() * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    std::vector<SortEncode> enc(n_keys);
    std::vector<uint32_t> width(n_keys);
    uint32_t total_bits = 0;
    for (int k = n_keys - 1; k >= 0; k--) {                 // the last key is the least significant
        if (mm[3 * k + 2] & 4)
            return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "sort_indices: key %d holds a string code >= n_codes (%lld)", k, (long long)n_codes);
        uint64_t mn = mm[3 * k], mx = mm[3 * k + 1];
        if (mn > mx) mn = mx = 0;                           // no number at all (nulls / NaNs only)
        SortEncode &e = enc[k];
        e.d = kd[k];
        e.asc = ascending ? (ascending[k] != 0) : 1;
        e.base = e.asc ? mn : mx;
        e.span = mx - mn;
        e.has_nan = (mm[3 * k + 2] & 2) ? 1 : 0;
        const unsigned __int128 top = (unsigned __int128)e.span + e.has_nan + ((mm[3 * k + 2] & 1) ? 1 : 0);
        uint32_t bits = 0;
        while (bits < 128 && (top >> bits) != 0) bits++;
        e.off = total_bits;
        e.n = n_rows;
        e.width = bits;
        width[k] = bits;
        total_bits += bits;
    }
    const uint32_t W = (total_bits + 63) / 64;
    if (W == 0) {                                           // every key constant: the identity permutation
        if (own_work) {
            ST_TRY(c->work.ensure(own_work + 4096, c->stream));
            if (!d_out && !(d_out = c->work.take<int64_t>(n))) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (sort)");
        }
        PhaseTimer pt(c, PANDRS_HIP_PHASE_SCATTER);
        hipLaunchKernelGGL(sort_iota_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, n_rows, d_out);
        HIP_TRY(hipGetLastError());
    } else {
        // ---- workspace, sized up front: codes [W][S] | second key buffer | two row buffers | counts | offsets | scan | and/or ----
        const uint32_t G = sort_grid(c, n_rows);
        const int64_t tiles = (n_rows + SORT_TILE - 1) / SORT_TILE;
        const int64_t rows_per_block = ((tiles + G - 1) / G) * SORT_TILE;
        const size_t n_counts = (size_t)SORT_MAX_BUCKETS * G;
        const size_t S = (n + 31) & ~size_t(31);            // word stride in rows (whole 256-byte pieces)
        ST_TRY(c->work.ensure(sort_order_workspace(c, n_rows, W) + own_work, c->stream));
        if (!d_out && !(d_out = c->work.take<int64_t>(n))) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (sort)");
        uint64_t *words = c->work.take<uint64_t>((size_t)W * S);
        uint64_t *kbuf = c->work.take<uint64_t>(n);
        uint32_t *rA = c->work.take<uint32_t>(n), *rB = c->work.take<uint32_t>(n);
        uint32_t *counts = c->work.take<uint32_t>(n_counts), *offs = c->work.take<uint32_t>(n_counts + 1);   // (+1: the scan writes its total at [n])
        uint32_t *seg = c->work.take<uint32_t>(scan_seg_count(n_counts));
        uint64_t *andor = c->work.take<uint64_t>((size_t)W * 2);
        if (!words || !kbuf || !rA || !rB || !counts || !offs || !seg || !andor)
            return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (sort)");
        std::vector<uint64_t> ao(2 * (size_t)W);
        {
            PhaseTimer pt(c, PANDRS_HIP_PHASE_OTHER);
            std::vector<bool> written(W, false);
            for (int k = n_keys - 1; k >= 0; k--) {
                SortEncode e = enc[k];
                if (width[k] == 0) continue;                // a constant key adds nothing to the order
                const uint32_t j0 = e.off >> 6, j1 = (e.off + width[k] - 1) >> 6;
                e.fresh = 0;
                for (uint32_t j = j0; j <= j1; j++)
                    if (!written[j]) { e.fresh |= 1u << (j - j0); written[j] = true; }
                e.W = W;
                e.words = words;
                e.stride = S;
                hipLaunchKernelGGL(sort_encode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, e);
            }
            HIP_TRY(hipGetLastError());
            for (uint32_t j = 0; j < W; j++) { ao[2 * j] = ~0ull; ao[2 * j + 1] = 0; }
            HIP_TRY(hipMemcpyAsync(andor, ao.data(), ao.size() * 8, hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(sort_word_andor_kernel, dim3(blocks_rd), dim3(256), 0, c->stream, words, S, W, n_rows, andor);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(ao.data(), andor, ao.size() * 8, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        // ---- the digit plan: per word, only the range of bits that vary; digits of <= SORT_MAX_DIGIT bits ----
        std::vector<SortDigit> plan;
        const uint32_t max_digit = c->opt.sort_digit_bits ? (uint32_t)std::clamp<int64_t>(c->opt.sort_digit_bits, 4, SORT_MAX_DIGIT) : SORT_MAX_DIGIT;
        for (uint32_t j = 0; j < W; j++) {
            const uint64_t vary = ao[2 * j] ^ ao[2 * j + 1];
            if (!vary) continue;
            const uint32_t lo = (uint32_t)__builtin_ctzll(vary), hi = 63 - (uint32_t)__builtin_clzll(vary);
            const uint32_t bits = hi - lo + 1, np = (bits + max_digit - 1) / max_digit, db = (bits + np - 1) / np;
            for (uint32_t q = 0; q < np; q++) {
                const uint32_t sh = lo + q * db, w = std::min(db, hi + 1 - sh);
                const uint64_t m = (w >= 64 ? ~0ull : ((1ull << w) - 1)) << sh;
                if (vary & m) plan.push_back(SortDigit{j, sh, w});   // a digit of constant bits orders nothing
            }
        }
        if (plan.empty()) {                                 // (a guard: W > 0 means some code varies)
            hipLaunchKernelGGL(sort_iota_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, n_rows, d_out);
            HIP_TRY(hipGetLastError());
        }
        // ---- the passes ----
        int64_t alg = 0;
        const uint32_t *rcur = nullptr;                     // nullptr: rows in input order (nothing scattered yet)
        uint32_t *rnext = rA;
        uint64_t *kcur = nullptr;
        for (size_t q = 0; q < plan.size(); q++) {
            const SortDigit &dg = plan[q];
            const bool last = q + 1 == plan.size();
            const bool first_of_word = q == 0 || plan[q - 1].word != dg.word;
            const bool last_of_word = last || plan[q + 1].word != dg.word;
            uint64_t *wj = words + (size_t)dg.word * S;
            if (first_of_word) {
                kcur = wj;
                if (rcur) {                                 // a higher word, in the order the lower words left
                    PhaseTimer pt(c, PANDRS_HIP_PHASE_GATHER);
                    hipLaunchKernelGGL(sort_regather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                                       wj, rcur, n_rows, kbuf);
                    HIP_TRY(hipGetLastError());
                    kcur = kbuf;
                    alg += (int64_t)n * 20;
                }
            }
            SortPass sp{};
            sp.kin = kcur;
            sp.rin = rcur;
            sp.n = n_rows; sp.rows_per_block = rows_per_block; sp.G = G; sp.shift = dg.shift; sp.dbits = dg.dbits;
            sp.counts = counts; sp.offs = offs;
            {
                PhaseTimer pt(c, PANDRS_HIP_PHASE_HISTOGRAM);
                hipLaunchKernelGGL(sort_hist_kernel, dim3(G), dim3(SORT_HIST_THREADS), 0, c->stream, sp);
                HIP_TRY(hipGetLastError());
            }
            {
                PhaseTimer pt(c, PANDRS_HIP_PHASE_SCAN);
                ST_TRY(exclusive_scan_u32(c, counts, (size_t)(1u << dg.dbits) * G, offs, seg));
            }
            {
                PhaseTimer pt(c, PANDRS_HIP_PHASE_SCATTER);
                if (last) {
                    sp.rout64 = d_out;
                    hipLaunchKernelGGL(sort_scatter_kernel<true>, dim3(G), dim3(SORT_THREADS), 0, c->stream, sp);
                } else {
                    // the word's keys are needed again only by its next digit: ping-pong between the word's slot and kbuf
                    sp.kout = last_of_word ? nullptr : (kcur == kbuf ? wj : kbuf);
                    sp.rout = rnext;
                    hipLaunchKernelGGL(sort_scatter_kernel<false>, dim3(G), dim3(SORT_THREADS), 0, c->stream, sp);
                    kcur = sp.kout;
                    rcur = rnext;
                    rnext = rnext == rA ? rB : rA;
                }
                HIP_TRY(hipGetLastError());
            }
            alg += (int64_t)n * (8 + 8 + (sp.rin ? 4 : 0) + (last ? 8 : 4 + (last_of_word ? 0 : 8)));
        }
        c->timings.algorithmic_bytes = alg;
        c->timings.n_partitions = (int64_t)plan.size();
    }
    if (perm_out) *perm_out = d_out;
    return 0;
}

int32_t sort_indices_entry(pandrs_hip_ctx *c, int32_t mem_space, const pandrs_hip_column *keys, int32_t n_keys,
                           const int32_t *ascending, const uint32_t *code_rank, int64_t n_codes, int64_t n_rows,
                           int32_t out_mem_space, int64_t *out_idx) {
    if (!c || !keys || n_keys <= 0 || n_rows < 0 || n_codes < 0 || (n_rows > 0 && !out_idx))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "sort_indices: bad arguments");
    ST_TRY(check_mem_space("sort_indices", mem_space, out_mem_space));
    if (n_rows >= (int64_t(1) << 32))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "sort_indices: %lld rows; one call takes fewer than 2^32", (long long)n_rows);
    bool any_string = false;
    for (int k = 0; k < n_keys; k++) {
        const int dt = keys[k].dtype;
        if (dt < PANDRS_HIP_I64 || dt > PANDRS_HIP_BOOLBITS)
            return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "sort_indices: key %d has dtype %d (CELL64 is not a frame column type)", k, dt);
        if (dt == PANDRS_HIP_U32CODE && (!code_rank || n_codes == 0))
            return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "sort_indices: string key %d needs the string-pool rank table (code_rank)", k);
        if (n_rows > 0 && !keys[k].data) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "sort_indices: key %d has no data", k);
        any_string |= dt == PANDRS_HIP_U32CODE;
    }
    if (n_rows == 0) return 0;
    std::lock_guard<std::mutex> lock(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    timings_begin(c);
    const size_t n = (size_t)n_rows;

    // ---- host columns (and the rank table with them) are staged; device columns are read in place ----
    std::vector<KeyDesc> kd(n_keys);
    const uint32_t *d_rank = nullptr;
    int64_t *d_out = nullptr;
    Stager stg{c, mem_space, out_mem_space};
    {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_STAGE_IN);
        const size_t rank_bytes = any_string ? (size_t)n_codes * 4 : 0;
        size_t need = stg.in_size(code_rank, rank_bytes) + stg.out_size(out_idx, n * 8);
        for (int k = 0; k < n_keys; k++) need += stg.col_size(keys[k], n_rows);
        ST_TRY(stg.reserve(need));
        d_rank = (const uint32_t *)stg.in(code_rank, rank_bytes);
        for (int k = 0; k < n_keys; k++) {
            const ColView v = stg.col(keys[k], n_rows);
            kd[k] = KeyDesc{v.data, v.mask, nullptr, keys[k].dtype};
        }
        d_out = stg.out(out_idx, n * 8);
        if (stg.status) return stg.status;
    }
    ST_TRY(sort_order_device(c, kd.data(), n_keys, ascending, d_rank, n_codes, n_rows, d_out, 0, nullptr));
    ST_TRY(stg.copy_back(n * 8));
    ST_TRY(timings_end(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace pandrs
