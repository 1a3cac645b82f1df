// filter.hip — stream compaction behind OptimizedDataFrame::filter / filter_rows / par_filter / select_by_mask
// (reference src/optimized/split_dataframe/data_ops.rs:37-121, row_ops.rs:26-130, parallel.rs:21-230,
// select.rs:150-167), gfx950, wave64.
//
// Row i is selected iff the BOOLBITS condition is Some(true): value bit set, null bit clear.
// 1. Selection (filter_select_kernel): one wave per 4096-row tile loads the condition and its null mask as whole
//    64-bit words, one word per lane, keeps sel = value & ~null (bits past the last row cleared) in the context and
//    writes the tile's popcount.  One exclusive scan of the tile counts (exclusive_scan_u32) gives every tile its
//    output offset; the scan's total is the selected row count.  Reduce-then-scan: every hand-off between
//    workgroups is a kernel boundary, no workgroup waits on another.
// 2. Compaction (filter_compact_kernel): one workgroup per tile.  The selection word of 64 consecutive rows is the
//    wave64 ballot of "this lane's row is selected", so a selected row's rank inside the tile is the exclusive
//    prefix of the tile's word popcounts plus mbcnt(word).  Each lane loads its selected rows' values (unselected
//    rows issue no load; nulls take the fill value), writes them to their rank in LDS, and the workgroup then
//    stores the tile's compacted run to out[offset[tile] ...) in consecutive, 64-byte-line-aligned stores.  Row
//    indices (filter_indices) are the same kernel with the row number as the value.
#include "engine.hpp"

#include <algorithm>

namespace pandrs {

constexpr int FT_THREADS = 256;                 // 4 waves
constexpr int FT_WORDS = 64;                    // selection words per tile
constexpr int FT_ROWS = FT_WORDS * 64;          // 4096 rows per tile
constexpr int FT_STEPS = FT_WORDS / (FT_THREADS / 64);   // words each wave ranks in a tile (16)

// whole 64-bit word `w` of a bit-packed array of nbytes bytes; the last, partial word and unaligned arrays byte by byte
__device__ __forceinline__ uint64_t ft_word(const uint8_t *p, int64_t w, int64_t nbytes) {
    const int64_t b = w * 8;
    if (b + 8 <= nbytes && (reinterpret_cast<uintptr_t>(p) & 7) == 0) return *reinterpret_cast<const uint64_t *>(p + b);
    uint64_t v = 0;
    for (int k = 0; k < 8; k++)
        if (b + k < nbytes) v |= (uint64_t)p[b + k] << (8 * k);
    return v;
}

__global__ __launch_bounds__(FT_THREADS) void filter_select_kernel(const uint8_t *cond, const uint8_t *cond_null, int64_t n_rows,
                                                                    int64_t n_tiles, uint64_t *sel, uint32_t *counts) {
    const int64_t tile = (int64_t)blockIdx.x * (FT_THREADS / 64) + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;                                 // (whole waves)
    const int64_t w = tile * FT_WORDS + (threadIdx.x & 63);
    const int64_t n_words = (n_rows + 63) / 64, nbytes = (n_rows + 7) / 8;
    uint64_t m = 0;
    if (w < n_words) {
        m = ft_word(cond, w, nbytes);
        if (cond_null) m &= ~ft_word(cond_null, w, nbytes);
        const int64_t left = n_rows - w * 64;
        if (left < 64) m &= (1ull << left) - 1;
        sel[w] = m;
    }
    uint32_t c = (uint32_t)__popcll(m);
    for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) counts[tile] = c;
}

// KIND 0: 8-byte values, 1: 4-byte, 2: bit-packed source -> one 0 / 1 byte per row, 3: the row index (int64)
template <int KIND> struct FtType { using T = uint64_t; };
template <> struct FtType<1> { using T = uint32_t; };
template <> struct FtType<2> { using T = uint8_t; };
template <> struct FtType<3> { using T = int64_t; };

template <int KIND>
__global__ __launch_bounds__(FT_THREADS) void filter_compact_kernel(const uint64_t *sel, const uint32_t *offs, int64_t n_rows,
                                                                     const void *src, const uint8_t *src_null, uint64_t fill, void *out) {
    using T = typename FtType<KIND>::T;
    __shared__ uint64_t s_sel[FT_WORDS], s_null[FT_WORDS], s_bits[FT_WORDS];
    __shared__ uint32_t s_pre[FT_WORDS];
    __shared__ T stage[FT_ROWS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t tile = blockIdx.x, base = tile * FT_ROWS;
    const int64_t n_words = (n_rows + 63) / 64, nbytes = (n_rows + 7) / 8;
    const int64_t w = tile * FT_WORDS + lane;
    if (wave == 0) {
        const uint64_t m = w < n_words ? sel[w] : 0;
        s_sel[lane] = m;
        const uint32_t pc = (uint32_t)__popcll(m);
        uint32_t inc = pc;                                      // inclusive prefix of the word popcounts
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(inc, o, 64);
            if (lane >= o) inc += u;
        }
        s_pre[lane] = inc - pc;
    } else if (wave == 1) {
        s_null[lane] = (src_null && w < n_words) ? ft_word(src_null, w, nbytes) : 0;
    } else if (wave == 2 && KIND == 2) {
        s_bits[lane] = w < n_words ? ft_word(static_cast<const uint8_t *>(src), w, nbytes) : 0;
    }
    __syncthreads();
    const uint32_t cnt = s_pre[FT_WORDS - 1] + (uint32_t)__popcll(s_sel[FT_WORDS - 1]);
    if (cnt == 0) return;                                       // (uniform)

    T v[FT_STEPS];
#pragma unroll
    for (int s = 0; s < FT_STEPS; s++) {
        const int j = s * (FT_THREADS / 64) + wave;
        const int64_t row = base + (int64_t)j * 64 + lane;
        v[s] = 0;
        if ((s_sel[j] >> lane) & 1) {
            if (KIND == 3) v[s] = (T)row;
            else if ((s_null[j] >> lane) & 1) v[s] = (T)fill;
            else if (KIND == 2) v[s] = (T)((s_bits[j] >> lane) & 1);
            else v[s] = __builtin_nontemporal_load(static_cast<const T *>(src) + row);
        }
    }
#pragma unroll
    for (int s = 0; s < FT_STEPS; s++) {
        const int j = s * (FT_THREADS / 64) + wave;
        const uint64_t m = s_sel[j];                            // == __ballot(selected) of this wave over row word j
        if ((m >> lane) & 1) {
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            stage[s_pre[j] + rank] = v[s];
        }
    }
    __syncthreads();
    // the tile's run, stored from the 64-byte line that holds its first element: every wave store covers whole lines
    constexpr int LINE = 64 / (int)sizeof(T);
    const int64_t o0 = offs[tile];
    const int lead = (int)(o0 & (LINE - 1));
    T *dst = static_cast<T *>(out) + o0;
    for (int k = t - lead; k < (int)cnt; k += FT_THREADS)
        if (k >= 0) dst[k] = stage[k];
}

namespace {

int kind_of(int32_t dtype) { return dtype == PANDRS_HIP_U32CODE ? 1 : (dtype == PANDRS_HIP_BOOLBITS ? 2 : 0); }
size_t elem_bytes(int kind) { return kind == 0 || kind == 3 ? 8 : (kind == 1 ? 4 : 1); }

int32_t launch_compact(pandrs_hip_ctx *c, int kind, const void *src, const uint8_t *src_null, uint64_t fill, void *out) {
    const FilterResult &f = c->fl;
    if (f.n_tiles == 0) return 0;
    const dim3 grid((unsigned)f.n_tiles), block(FT_THREADS);
    switch (kind) {
    case 0: hipLaunchKernelGGL(filter_compact_kernel<0>, grid, block, 0, c->stream, f.sel, f.offs, f.n_rows, src, src_null, fill, out); break;
    case 1: hipLaunchKernelGGL(filter_compact_kernel<1>, grid, block, 0, c->stream, f.sel, f.offs, f.n_rows, src, src_null, fill, out); break;
    case 2: hipLaunchKernelGGL(filter_compact_kernel<2>, grid, block, 0, c->stream, f.sel, f.offs, f.n_rows, src, src_null, fill, out); break;
    default: hipLaunchKernelGGL(filter_compact_kernel<3>, grid, block, 0, c->stream, f.sel, f.offs, f.n_rows, src, src_null, fill, out); break;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

size_t filter_workspace_bytes(int64_t n_rows) {
    const size_t words = (size_t)(n_rows + 63) / 64, tiles = (size_t)(n_rows + FT_ROWS - 1) / FT_ROWS;
    return Arena::padded(words * 8 + 16) + 2 * Arena::padded((tiles + 1) * 4) + Arena::padded(scan_seg_count(tiles + 1) * 4) + 4096;
}

int32_t filter_indices_entry(pandrs_hip_ctx *c, int32_t mem_space, const pandrs_hip_column *cond, int64_t n_rows,
                             int32_t out_mem_space, int64_t *out_idx, int64_t *out_count) {
    if (!c || !cond || n_rows < 0 || !out_count || (n_rows > 0 && !cond->data))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "filter_indices: bad arguments");
    ST_TRY(check_mem_space("filter_indices", mem_space, out_idx ? out_mem_space : PANDRS_HIP_MEM_DEVICE));    // (no output, no output space)
    if (cond->dtype != PANDRS_HIP_BOOLBITS)
        return fail(PANDRS_HIP_ERR_TYPE_MISMATCH, "filter_indices: the condition has dtype %d, expected BOOLBITS (Boolean)", cond->dtype);
    if (n_rows >= (int64_t(1) << 32))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "filter_indices: %lld rows; one call takes fewer than 2^32", (long long)n_rows);
    std::lock_guard<std::mutex> lock(c->mu);
    FilterResult &f = c->fl;
    f.valid = false;                                            // the previous selection is gone whatever happens below
    *out_count = 0;
    HIP_TRY(hipSetDevice(c->device));
    timings_begin(c);
    const int64_t n_words = (n_rows + 63) / 64, n_tiles = (n_rows + FT_ROWS - 1) / FT_ROWS;
    const size_t nbytes = (size_t)(n_rows + 7) / 8;
    // ---- the retained selection: sel words | tile counts | tile offsets (+ total) | scan scratch, sized up front ----
    ST_TRY(c->filt.ensure(filter_workspace_bytes(n_rows), c->stream));
    f.sel = c->filt.take<uint64_t>((size_t)n_words + 2);
    uint32_t *counts = c->filt.take<uint32_t>((size_t)n_tiles + 1);
    f.offs = c->filt.take<uint32_t>((size_t)n_tiles + 1);
    uint32_t *seg = c->filt.take<uint32_t>(scan_seg_count((size_t)n_tiles + 1));
    if (!f.sel || !counts || !f.offs || !seg) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (filter)");
    f.n_rows = n_rows;
    f.n_tiles = n_tiles;
    f.n_selected = 0;
    if (n_rows == 0) { f.valid = true; return timings_end(c); }

    ColView cv{cond->data, cond->null_mask};
    int64_t *d_out = out_idx;
    Stager stg{c, mem_space, out_mem_space};
    const size_t out_room = (size_t)n_rows * 8;         // (the count is not known yet: room for every row)
    if (const size_t need = stg.col_size(*cond, n_rows) + stg.out_size(out_idx, out_room)) {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_STAGE_IN);
        ST_TRY(stg.reserve(need));
        cv = stg.col(*cond, n_rows);
        d_out = stg.out(out_idx, out_room);
        if (stg.status) return stg.status;
    }
    const uint8_t *d_cond = static_cast<const uint8_t *>(cv.data), *d_null = cv.mask;
    {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_OTHER);
        const int64_t blocks = (n_tiles + FT_THREADS / 64 - 1) / (FT_THREADS / 64);
        hipLaunchKernelGGL(filter_select_kernel, dim3((unsigned)blocks), dim3(FT_THREADS), 0, c->stream, d_cond, d_null, n_rows, n_tiles,
                           f.sel, counts);
        HIP_TRY(hipGetLastError());
        ST_TRY(exclusive_scan_u32(c, counts, (size_t)n_tiles, f.offs, seg));
    }
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, f.offs + n_tiles, 4, hipMemcpyDeviceToHost, c->stream));
    if (out_idx) {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_SCATTER);
        f.valid = true;
        ST_TRY(launch_compact(c, 3, nullptr, nullptr, 0, d_out));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    f.n_selected = total;
    f.valid = true;
    if (stg.out_dev && total) {
        ST_TRY(stg.copy_back((size_t)total * 8));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    c->timings.algorithmic_bytes = (int64_t)nbytes * (d_null ? 3 : 2) + (out_idx ? (int64_t)total * 8 : 0);
    *out_count = total;
    return timings_end(c);
}

int32_t filter_gather_entry(pandrs_hip_ctx *c, int32_t src_mem_space, const pandrs_hip_column *src, int64_t n_src, uint64_t fill_bits,
                            int32_t out_mem_space, void *out) {
    if (!c || !src || n_src < 0) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "filter_gather: bad arguments");
    ST_TRY(check_mem_space("filter_gather", src_mem_space, out_mem_space));
    if (src->dtype < PANDRS_HIP_I64 || src->dtype > PANDRS_HIP_BOOLBITS)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "filter_gather: bad dtype %d (CELL64 is not a frame column type)", src->dtype);
    std::lock_guard<std::mutex> lock(c->mu);                    // one critical section: the selection and the staging live in the context
    const FilterResult &f = c->fl;
    if (!f.valid) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "filter_gather: no selection retained in this context (call pandrs_hip_filter_indices first)");
    if (n_src != f.n_rows)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "filter_gather: the column has %lld rows, the selection %lld", (long long)n_src,
                    (long long)f.n_rows);
    const int64_t n = f.n_selected;
    if (n == 0) return 0;
    if (!out || !src->data) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "filter_gather: null column data or output");
    const int kind = kind_of(src->dtype);
    const size_t esz = elem_bytes(kind), sbytes = dtype_bytes(src->dtype, n_src), mbytes = (size_t)(n_src + 7) / 8;
    HIP_TRY(hipSetDevice(c->device));
    timings_begin(c);
    ColView sv{src->data, src->null_mask};
    void *d_out = out;
    Stager stg{c, src_mem_space, out_mem_space};
    if (const size_t need = stg.col_size(*src, n_src) + stg.out_size(out, (size_t)n * esz)) {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_STAGE_IN);
        ST_TRY(stg.reserve(need));
        sv = stg.col(*src, n_src);
        d_out = stg.out(out, (size_t)n * esz);
        if (stg.status) return stg.status;
    }
    const void *d_src = sv.data;
    const uint8_t *d_null = sv.mask;
    if (kind != 2 && (reinterpret_cast<uintptr_t>(d_src) & (esz - 1)))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "filter_gather: the column must be %zu-byte aligned", esz);
    {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_GATHER);
        ST_TRY(launch_compact(c, kind, d_src, d_null, fill_bits, d_out));
    }
    ST_TRY(stg.copy_back((size_t)n * esz));
    c->timings.algorithmic_bytes = (int64_t)(kind == 2 ? mbytes : sbytes) + (d_null ? (int64_t)mbytes : 0) + (int64_t)(mbytes + n * esz);
    ST_TRY(timings_end(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace pandrs
