// distinct.hip — the distinct values of one column and how often each occurs, behind PandasCompatExt::value_counts / unique /
// nunique / mode / is_unique (reference src/dataframe/pandas_compat/functions.rs:343-384, :775-788, :1709-1753, :4120-4139,
// :4226-4259), gfx950, wave64.  pandrs_hip.h states the contract: one entry per distinct number, then at most one NaN entry and
// one NULL entry; counts are exact int64; a cell under a null bit is never looked at.
// 1. Census: one stream over the column in tiles of DN_TILE rows (16-byte loads of 8-byte cells): min and max of the cells'
//    order image, the NaN / null / valid counts, and for F64 whether every number is integral with |v| <= 2^53 and whether
//    a -0.0 is present.  One read-back.
// 2. Direct path, when max - min + 1 <= DN_MAX_CELLS: a second stream counts cell - min into a uint32 table in LDS (lanes of a
//    wave holding the same cell add once by ballot, the rest by LDS atomics: a hot value does not serialise); a workgroup adds
//    its non-zero cells to 64-bit workspace counters when it ends; one small workgroup compacts the non-zero cells in ascending
//    cell order into the entry list.  No workgroup waits for another.
// 3. Engine path, everything else: the groupby engine runs with the column as the key and COUNT; a kernel turns its groups
//    (all NaNs one cell, the NULL group) into entries.
// 4. Finish, both paths: every entry carries the int64 order key of its value; the stable radix sort of sort.hip orders the
//    entries (count descending, then class, then value) unless the direct table is already in order; a gather writes the
//    retained list; two small kernels find the largest count among the numbers and how many entries have it.
#include "distinct.hpp"

#include <algorithm>

namespace pandrs {

constexpr int DN_THREADS = 256;
constexpr int DN_LOADS = 4;                              // 16-byte loads in flight per thread
constexpr int DN_TILE = DN_THREADS * DN_LOADS * 2;       // rows per workgroup iteration (2048; pandrs_hip.h: distinct_tile_rows)
constexpr int DN_BLOCKS_PER_CU = 4;                      // pandrs_hip.h: distinct_blocks_per_cu
constexpr int DN_MAX_CELLS = 8192;                       // pandrs_hip.h: distinct_direct_max_cells; 32 KiB of uint32 counters per workgroup
constexpr int DN_PEEL = 4;                               // cells a wave folds by ballot before plain atomics
constexpr int DN_PEEL_MIN = 4;                           // ... as long as a round folds at least this many lanes
constexpr int DN_COMPACT_THREADS = 256;
static_assert(DN_MAX_CELLS % DN_COMPACT_THREADS == 0, "the compaction gives every thread the same number of consecutive cells");

// census[] arrives as {~0, 0, 0, 0, 0, 0}
template <int DT>
__global__ __launch_bounds__(DN_THREADS) void dn_census_kernel(DnCol c, unsigned long long *census) {
    dn_census<DT, DN_THREADS, DN_LOADS>(c, census);
}

// lanes holding the same cell as the first pending lane add their number in one LDS atomic (the idiom of bin.hip's bin_count)
__device__ __forceinline__ void dn_count(uint32_t *h, bool m, uint32_t key) {
    uint64_t todo = __ballot(m);
    const uint32_t lane = threadIdx.x & 63;
    for (int round = 0; todo && round < DN_PEEL; round++) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint32_t k0 = __shfl(key, leader, 64);
        const uint64_t same = __ballot(m && key == k0) & todo;
        if (lane == (uint32_t)leader) atomicAdd(&h[k0], (uint32_t)__popcll(same));
        todo &= ~same;
        if (__popcll(same) < DN_PEEL_MIN) break;        // few lanes share a cell: the rest add on their own
    }
    if ((todo >> lane) & 1) atomicAdd(&h[key], 1u);
}

// dynamic LDS: n_cells uint32 counters.  counters[] (n_cells 64-bit words) arrives zeroed.  NaN and null cells are skipped:
// their counts are the census's.
template <int DT>
__global__ __launch_bounds__(DN_THREADS) void dn_direct_kernel(DnCol c, uint64_t base, uint32_t n_cells, unsigned long long *counters) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dn_smem[];
    uint32_t *h = reinterpret_cast<uint32_t *>(dn_smem);
    for (uint32_t i = threadIdx.x; i < n_cells; i += DN_THREADS) h[i] = 0;
    __syncthreads();
    const bool aligned = (reinterpret_cast<uintptr_t>(c.data) & 15) == 0;
    const int64_t tiles = (c.n + DN_TILE - 1) / DN_TILE;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t r0 = t * DN_TILE + 2 * (int64_t)threadIdx.x;
        uint64_t v[DN_LOADS][2];
        uint32_t in[DN_LOADS], nul[DN_LOADS];
#pragma unroll
        for (int k = 0; k < DN_LOADS; k++) {                 // every load of the tile in flight before the first count
            const int64_t r = r0 + (int64_t)k * 2 * DN_THREADS;
            dn_load2<DT>(c, r, aligned, v[k], in[k]);
            nul[k] = c.null && in[k] ? ((uint32_t)c.null[r >> 3] >> (r & 7)) & 3 : 0;
        }
#pragma unroll
        for (int k = 0; k < DN_LOADS; k++)                   // (a uniform loop: the ballots of dn_count see every lane)
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const uint64_t b = v[k][j];
                bool m = ((in[k] >> j) & 1) && !((nul[k] >> j) & 1);
                if (DT == PANDRS_HIP_F64) m = m && !dn_is_nan(b);
                const uint64_t idx = m ? dn_cell_index<DT>(b, base) : 0;
                m = m && idx < (uint64_t)n_cells;            // (the census bounds every number: a guard, not a path)
                dn_count(h, m, (uint32_t)idx);
            }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_cells; i += DN_THREADS)
        if (h[i]) atomicAdd(&counters[i], (unsigned long long)h[i]);
}

// the entry lists: value cell, flag (0 number, 1 NaN, 2 NULL), count, and the sort keys (flag and order key as int64 columns)
struct DnList {
    uint64_t *values;
    uint8_t *flags;
    int64_t *counts;
    int64_t *cls;        // the flag as an int64 sort key
    int64_t *ord;        // ascending in the value order; 0 for NaN / NULL
};

__device__ __forceinline__ void dn_emit(const DnList &o, size_t at, uint64_t value, uint32_t flag, int64_t count, int64_t ord) {
    o.values[at] = value; o.flags[at] = (uint8_t)flag; o.counts[at] = count; o.cls[at] = (int64_t)flag; o.ord[at] = ord;
}

// One workgroup: the non-zero cells of the direct table in ascending cell order, then the NaN and the NULL entry.
template <int DT>
__global__ __launch_bounds__(DN_COMPACT_THREADS) void dn_compact_kernel(const unsigned long long *counters, uint32_t n_cells, uint64_t base,
                                                                        int64_t n_nan, int64_t n_null, DnRank rk, DnList o,
                                                                        unsigned long long *n_entries) {
    __shared__ uint32_t wave_tot[17];
    const uint32_t per = (n_cells + DN_COMPACT_THREADS - 1) / DN_COMPACT_THREADS;
    const uint32_t lo = min(threadIdx.x * per, n_cells), hi = min(lo + per, n_cells);
    uint32_t mine = 0;
    for (uint32_t i = lo; i < hi; i++) mine += counters[i] ? 1u : 0u;
    uint32_t total = 0;
    uint32_t at = block_exclusive_scan<DN_COMPACT_THREADS>(mine, wave_tot, &total);
    for (uint32_t i = lo; i < hi; i++) {
        const unsigned long long n = counters[i];
        if (!n) continue;
        const uint64_t number = base + i;                                   // I64 / code / bool: the cell; F64: the integer
        const uint64_t cell = DT == PANDRS_HIP_F64 ? (uint64_t)__double_as_longlong((double)(int64_t)number) : number;
        dn_emit(o, at++, cell, 0, (int64_t)n, dn_order_key<DT>(cell, rk));
    }
    if (threadIdx.x == 0) {
        uint32_t e = total;
        if (n_nan) dn_emit(o, e++, CANON_NAN, 1, n_nan, 0);
        if (n_null) dn_emit(o, e++, 0, 2, n_null, 0);
        *n_entries = e;
    }
}

// the engine's groups -> entries: the NULL group by its null byte, the NaN group by any NaN cell (written as the canonical one)
template <int DT>
__global__ void dn_from_groups_kernel(const uint64_t *keys, const uint8_t *key_null, const double *counts, int64_t G, DnRank rk, DnList o) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const uint64_t cell = keys[g];
    const int64_t n = (int64_t)counts[g];                    // exact: a count below 2^32
    if (key_null[g]) dn_emit(o, g, 0, 2, n, 0);
    else if (DT == PANDRS_HIP_F64 && dn_is_nan(cell)) dn_emit(o, g, CANON_NAN, 1, n, 0);
    else dn_emit(o, g, cell, 0, n, dn_order_key<DT>(cell, rk));
}

__global__ void dn_gather_kernel(DnList in, const int64_t *perm, int64_t G, DnList out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= G) return;
    const int64_t s = perm[i];
    if (s < 0 || s >= G) return;                             // (a permutation of [0, G): a guard, not a path)
    out.values[i] = in.values[s]; out.flags[i] = in.flags[s]; out.counts[i] = in.counts[s];
}

// mode[0] (arrives 0) = the largest count among the numbers; mode[1] (arrives 0) = how many entries have it
__global__ void dn_max_count_kernel(const uint8_t *flags, const int64_t *counts, int64_t G, unsigned long long *mode) {
    unsigned long long m = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < G; i += (int64_t)gridDim.x * blockDim.x)
        if (!flags[i]) m = max(m, (unsigned long long)counts[i]);
    m = dn_wave_max(m);
    if ((threadIdx.x & 63) == 0 && m) atomicMax(&mode[0], m);
}
__global__ void dn_n_modes_kernel(const uint8_t *flags, const int64_t *counts, int64_t G, unsigned long long *mode) {
    const unsigned long long top = mode[0];
    unsigned long long k = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < G; i += (int64_t)gridDim.x * blockDim.x)
        if (!flags[i] && top && (unsigned long long)counts[i] == top) k++;
    k = dn_wave_sum(k);
    if ((threadIdx.x & 63) == 0 && k) atomicAdd(&mode[1], k);
}

static DnList dn_take_list(Arena &a, size_t cap, bool with_keys) {
    DnList l{};
    l.values = a.take<uint64_t>(cap);
    l.flags = a.take<uint8_t>(cap);
    l.counts = a.take<int64_t>(cap);
    if (with_keys) { l.cls = a.take<int64_t>(cap); l.ord = a.take<int64_t>(cap); }
    return l;
}
static size_t dn_list_bytes(size_t cap, bool with_keys) {
    return (with_keys ? 4 : 2) * Arena::padded(cap * 8) + Arena::padded(cap);
}

int32_t distinct_entry(pandrs_hip_ctx *c, int32_t mem_space, const pandrs_hip_column *col, int64_t n_rows, int32_t order,
                       const uint32_t *code_rank, int64_t n_codes, pandrs_hip_distinct_info *out_info) {
    if (!c || !col || !out_info || n_rows < 0 || n_codes < 0 || (n_rows > 0 && !col->data))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "distinct: bad arguments");
    ST_TRY(check_mem_space("distinct", mem_space));
    if (order != PANDRS_HIP_DISTINCT_BY_VALUE && order != PANDRS_HIP_DISTINCT_BY_COUNT)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "distinct: order %d (PANDRS_HIP_DISTINCT_BY_VALUE or PANDRS_HIP_DISTINCT_BY_COUNT)", order);
    const int dt = col->dtype;
    if (dt != PANDRS_HIP_I64 && dt != PANDRS_HIP_F64 && dt != PANDRS_HIP_U32CODE && dt != PANDRS_HIP_BOOLBITS)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "distinct: the column has dtype %d (I64, F64, U32CODE or BOOLBITS)", dt);
    if (code_rank && (dt != PANDRS_HIP_U32CODE || n_codes == 0))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "distinct: a rank table needs a U32CODE column and n_codes > 0");
    if (n_rows >= (int64_t(1) << 32))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "distinct: %lld rows; one call takes fewer than 2^32", (long long)n_rows);
    std::lock_guard<std::mutex> lock(c->mu);
    *out_info = pandrs_hip_distinct_info{};
    DistinctResult &res = c->dn;
    res = DistinctResult{};
    c->gb.valid = false;                                     // whichever path answers: one contract
    HIP_TRY(hipSetDevice(c->device));
    timings_begin(c);                                        // (drops the retained list: c->dn.valid)
    if (n_rows == 0) {                                       // an empty list, and a record of its own like any other call
        ST_TRY(timings_end(c));
        res.valid = true;
        return 0;
    }
    const bool check_codes = dt == PANDRS_HIP_U32CODE && n_codes > 0;

    ColView cv{col->data, col->null_mask};
    const uint32_t *d_rank = code_rank;
    Stager stg{c, mem_space};
    const size_t rank_bytes = code_rank ? (size_t)n_codes * 4 : 0;
    if (const size_t need = stg.col_size(*col, n_rows) + stg.in_size(code_rank, rank_bytes)) {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_STAGE_IN);
        ST_TRY(stg.reserve(need));
        cv = stg.col(*col, n_rows);
        d_rank = static_cast<const uint32_t *>(stg.in(code_rank, rank_bytes));
        if (stg.status) return stg.status;
    }
    if ((dt == PANDRS_HIP_I64 || dt == PANDRS_HIP_F64) && (reinterpret_cast<uintptr_t>(cv.data) & 7))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "distinct: the column must be 8-byte aligned");
    if (dt == PANDRS_HIP_U32CODE && (reinterpret_cast<uintptr_t>(cv.data) & 3))
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "distinct: the codes must be 4-byte aligned");

    // ---- census.  The workspace of this stage and of the direct table does not grow with n_rows.
    const size_t head_bytes = Arena::padded(DN_CENSUS_WORDS * 8) + Arena::padded((size_t)DN_MAX_CELLS * 8) + Arena::padded(16);
    ST_TRY(c->work.ensure(head_bytes, c->stream));
    unsigned long long *d_census = c->work.take<unsigned long long>(DN_CENSUS_WORDS);
    unsigned long long *d_counters = c->work.take<unsigned long long>(DN_MAX_CELLS);
    unsigned long long *d_nent = c->work.take<unsigned long long>(2);
    if (!d_census || !d_counters || !d_nent) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (distinct)");
    const DnCol dc{cv.data, cv.mask, n_rows};
    const int64_t tiles = (n_rows + DN_TILE - 1) / DN_TILE;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)c->n_cu * DN_BLOCKS_PER_CU, tiles));
    uint64_t *pin = static_cast<uint64_t *>(c->pinned);
    uint64_t cs[DN_CENSUS_WORDS];
    {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_ESTIMATE);
        pin[DN_MIN] = ~0ull;
        for (int i = 1; i < DN_CENSUS_WORDS; i++) pin[i] = 0;
        HIP_TRY(hipMemcpyAsync(d_census, pin, DN_CENSUS_WORDS * 8, hipMemcpyHostToDevice, c->stream));
        DN_DISPATCH(dt, hipLaunchKernelGGL(dn_census_kernel<DT>, dim3(grid), dim3(DN_THREADS), 0, c->stream, dc, d_census));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(pin, d_census, DN_CENSUS_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        std::memcpy(cs, pin, sizeof cs);
    }
    const int64_t n_nan = (int64_t)cs[DN_NAN], n_null = (int64_t)cs[DN_NULL], n_valid = (int64_t)cs[DN_VALID];
    if (n_nan + n_null + n_valid != n_rows)
        return fail(PANDRS_HIP_ERR_COMPUTATION, "distinct: the census counted %lld of %lld rows", (long long)(n_nan + n_null + n_valid), (long long)n_rows);
    if (check_codes && n_valid && cs[DN_MAX] >= (uint64_t)n_codes)
        return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "distinct: the column holds a string code >= n_codes (%lld)", (long long)n_codes);

    // ---- which path: the numbers' span as a table.  base = the smallest number as the table counts it
    uint64_t base = 0, span = 0;                             // span = max - min in unsigned 64-bit; cells = span + 1 may be 2^64
    const bool can_direct = dn_span(dt, cs, &base, &span) && span < (uint64_t)DN_MAX_CELLS;
    const int64_t want = c->opt.distinct_path;               // 1: direct wherever possible; 2: always the engine; 0: direct wherever possible
    const bool direct = can_direct && want != 2;
    const DnRank rk{d_rank, (uint64_t)n_codes};

    DnList raw{};
    int64_t G = 0;
    bool in_order = false;                                   // the entries already stand in BY_VALUE order
    if (direct) {
        const uint32_t n_cells = (uint32_t)span + 1;
        ST_TRY(c->dn_arena.ensure(2 * dn_list_bytes((size_t)n_cells + 2, true), c->stream));
        raw = dn_take_list(c->dn_arena, (size_t)n_cells + 2, true);
        if (!raw.values || !raw.flags || !raw.counts || !raw.cls || !raw.ord) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (distinct)");
        {
            PhaseTimer pt(c, PANDRS_HIP_PHASE_AGGREGATE);
            HIP_TRY(hipMemsetAsync(d_counters, 0, (size_t)n_cells * 8, c->stream));
            DN_DISPATCH(dt, hipLaunchKernelGGL(dn_direct_kernel<DT>, dim3(grid), dim3(DN_THREADS), (size_t)n_cells * 4, c->stream, dc, base, n_cells, d_counters));
            HIP_TRY(hipGetLastError());
        }
        {
            PhaseTimer pt(c, PANDRS_HIP_PHASE_GATHER);
            DN_DISPATCH(dt, hipLaunchKernelGGL(dn_compact_kernel<DT>, dim3(1), dim3(DN_COMPACT_THREADS), 0, c->stream, d_counters, n_cells, base, n_nan, n_null, rk, raw, d_nent));
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(pin, d_nent, 8, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        G = (int64_t)pin[0];
        if (G < 0 || G > (int64_t)n_cells + 2) return fail(PANDRS_HIP_ERR_COMPUTATION, "distinct: %lld entries from %u cells", (long long)G, n_cells);
        in_order = !(dt == PANDRS_HIP_U32CODE && d_rank);
    } else {
        // the groupby engine with the column as the key and COUNT: its own estimate, paths and retries
        const pandrs_hip_agg_spec count{0, PANDRS_HIP_AGG_COUNT};
        Plan pl;
        const int32_t no_dtype = PANDRS_HIP_I64;              // (COUNT reads no value column: the plan has no source)
        const uint8_t no_nulls = 0;
        ST_TRY(build_plan(&no_dtype, &no_nulls, 1, &count, 1, pl));
        RowSource rs;
        rs.n_rows = n_rows;
        rs.key = KeyDesc{cv.data, cv.mask, nullptr, dt};
        c->jn.valid = false;                                 // the engine's result arena is the join result's
        ST_TRY(run_engine(c, rs, pl, /*merge=*/false, /*partials=*/false, 1, dt, 1));
        const GroupbyResult &g = c->gb;
        if (!g.valid) return fail(PANDRS_HIP_ERR_COMPUTATION, "distinct: the engine left no result");
        G = g.n_groups;
        ST_TRY(c->dn_arena.ensure(2 * dn_list_bytes((size_t)G + 2, true), c->stream));
        raw = dn_take_list(c->dn_arena, (size_t)G + 2, true);
        if (!raw.values || !raw.flags || !raw.counts || !raw.cls || !raw.ord) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (distinct)");
        if (G > 0) {
            PhaseTimer pt(c, PANDRS_HIP_PHASE_GATHER);
            DN_DISPATCH(dt, hipLaunchKernelGGL(dn_from_groups_kernel<DT>, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, c->stream, g.keys, g.key_null, g.aggs, G, rk, raw));
            HIP_TRY(hipGetLastError());
        }
        c->gb.valid = false;
    }

    // ---- finish: order, the retained list, the modes
    DnList fin = raw;
    const bool sorted_already = G <= 1 || (in_order && order == PANDRS_HIP_DISTINCT_BY_VALUE);
    if (!sorted_already) {
        fin = dn_take_list(c->dn_arena, (size_t)G + 2, false);
        if (!fin.values || !fin.flags || !fin.counts) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (distinct)");
        const KeyDesc keys[3] = {KeyDesc{raw.counts, nullptr, nullptr, PANDRS_HIP_I64}, KeyDesc{raw.cls, nullptr, nullptr, PANDRS_HIP_I64},
                                 KeyDesc{raw.ord, nullptr, nullptr, PANDRS_HIP_I64}};
        const int32_t asc[3] = {0, 1, 1};
        const bool by_count = order == PANDRS_HIP_DISTINCT_BY_COUNT;
        int64_t *perm = nullptr;
        ST_TRY(sort_order_device(c, by_count ? keys : keys + 1, by_count ? 3 : 2, by_count ? asc : asc + 1, nullptr, 0, G, nullptr, 4096, &perm));
        PhaseTimer pt(c, PANDRS_HIP_PHASE_GATHER);
        hipLaunchKernelGGL(dn_gather_kernel, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, c->stream, raw, perm, G, fin);
        HIP_TRY(hipGetLastError());
    }
    // (the head block is gone once the sort has sized c->work: the mode cells live beside the list)
    unsigned long long *d_mode = c->dn_arena.take<unsigned long long>(2);
    if (!d_mode) return fail(PANDRS_HIP_ERR_OUT_OF_MEMORY, "workspace too small (distinct)");
    {
        PhaseTimer pt(c, PANDRS_HIP_PHASE_OTHER);
        HIP_TRY(hipMemsetAsync(d_mode, 0, 16, c->stream));
        if (G > 0) {
            const int mg = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)c->n_cu * 4, (G + 255) / 256));
            hipLaunchKernelGGL(dn_max_count_kernel, dim3(mg), dim3(256), 0, c->stream, fin.flags, fin.counts, G, d_mode);
            hipLaunchKernelGGL(dn_n_modes_kernel, dim3(mg), dim3(256), 0, c->stream, fin.flags, fin.counts, G, d_mode);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(pin, d_mode, 16, hipMemcpyDeviceToHost, c->stream));
    }
    const int64_t by_path = direct ? 1 : 2;
    const int64_t alg = n_rows * (int64_t)(dt == PANDRS_HIP_U32CODE ? 4 : (dt == PANDRS_HIP_BOOLBITS ? 0 : 8)) + (cv.mask ? (n_rows + 7) / 8 : 0);
    ST_TRY(timings_end(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->timings.n_partitions = by_path;                       // which path answered: 1 = direct table, 2 = engine
    c->timings.algorithmic_bytes = (direct ? 2 : 1) * alg + G * 17;
    out_info->n_entries = G;
    out_info->n_valid = n_valid;
    out_info->nan_count = n_nan;
    out_info->null_count = n_null;
    out_info->max_count = (int64_t)pin[0];
    out_info->n_modes = (int64_t)pin[1];
    out_info->path = (int32_t)by_path;
    res.n_entries = G;
    res.values = fin.values; res.flags = fin.flags; res.counts = fin.counts;
    res.valid = true;
    return 0;
}

int32_t distinct_fetch_entry(pandrs_hip_ctx *c, int32_t out_mem_space, uint64_t *out_values, uint8_t *out_flags, int64_t *out_counts) {
    if (!c) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "distinct_fetch: no context");
    ST_TRY(check_mem_space("distinct_fetch", out_mem_space));
    std::lock_guard<std::mutex> lock(c->mu);
    const DistinctResult &r = c->dn;
    if (!r.valid) return fail(PANDRS_HIP_ERR_INVALID_ARGUMENT, "no distinct list retained in this context");
    const size_t n = (size_t)r.n_entries;
    if (!n) return 0;
    HIP_TRY(hipSetDevice(c->device));
    const hipMemcpyKind kind = out_mem_space == PANDRS_HIP_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (out_values) HIP_TRY(hipMemcpyAsync(out_values, r.values, n * 8, kind, c->stream));
    if (out_flags) HIP_TRY(hipMemcpyAsync(out_flags, r.flags, n, kind, c->stream));
    if (out_counts) HIP_TRY(hipMemcpyAsync(out_counts, r.counts, n * 8, kind, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace pandrs
