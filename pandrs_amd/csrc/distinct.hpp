// distinct.hpp — what distinct.hip and pivot.hip share: a key column as a stream of 8-byte cells, the order image of a cell, the
// census of a column (min and max image, NaN / null / valid counts, F64 integrality and -0.0 presence) and the order key an entry
// or a label sorts by.  Device code only; every tile size is a template parameter of its user.
#pragma once
#include "engine.hpp"

namespace pandrs {

struct DnCol {
    const void *data;         // I64 / F64: 8-byte aligned; U32CODE: 4-byte aligned; BOOLBITS: bytes
    const uint8_t *null;      // LSB-first, 1 = null, any byte offset
    int64_t n;
};

// the census block: [0] min image, [1] max image, [2] NaN cells, [3] null cells, [4] numbers, [5] flags
enum { DN_MIN = 0, DN_MAX, DN_NAN, DN_NULL, DN_VALID, DN_FLAGS, DN_CENSUS_WORDS };
constexpr uint64_t DN_F_FRACTION = 1;                    // F64: a number that is not integral or lies beyond +-2^53
constexpr uint64_t DN_F_NEGZERO = 2;                     // F64: a -0.0

__device__ __forceinline__ bool dn_is_nan(uint64_t b) { return (b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull; }

// The order image of a cell: unsigned, ascending in the value order of pandrs_hip.h (-0.0 before 0.0).
template <int DT>
__device__ __forceinline__ uint64_t dn_image(uint64_t cell) {
    if (DT == PANDRS_HIP_I64) return cell ^ 0x8000000000000000ull;
    if (DT == PANDRS_HIP_F64) return (cell >> 63) ? ~cell : (cell | 0x8000000000000000ull);
    return cell;
}

// rows r and r + 1 (r even) of the column as 8-byte cells; `in` says which of the two exist
template <int DT>
__device__ __forceinline__ void dn_load2(const DnCol &c, int64_t r, bool aligned, uint64_t v[2], uint32_t &in) {
    v[0] = v[1] = 0;
    in = r + 1 < c.n ? 3u : (r < c.n ? 1u : 0u);
    if (!in) return;
    if (DT == PANDRS_HIP_I64 || DT == PANDRS_HIP_F64) {
        const uint64_t *d = static_cast<const uint64_t *>(c.data);
        if (in == 3 && aligned) {
            const ulonglong2 q = *reinterpret_cast<const ulonglong2 *>(d + r);
            v[0] = q.x; v[1] = q.y;
        } else {
            v[0] = d[r];
            if (in == 3) v[1] = d[r + 1];
        }
    } else if (DT == PANDRS_HIP_U32CODE) {
        const uint32_t *d = static_cast<const uint32_t *>(c.data);
        if (in == 3 && (reinterpret_cast<uintptr_t>(d) & 7) == 0) {      // (r even: d + r is as aligned as d)
            const uint2 q = *reinterpret_cast<const uint2 *>(d + r);
            v[0] = q.x; v[1] = q.y;
        } else {
            v[0] = d[r];
            if (in == 3) v[1] = d[r + 1];
        }
    } else {
        const uint32_t b = static_cast<const uint8_t *>(c.data)[r >> 3] >> (r & 7);      // (r even: both bits lie in one byte)
        v[0] = b & 1; v[1] = (b >> 1) & 1;
    }
}

__device__ __forceinline__ uint64_t dn_wave_min(uint64_t v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) { const uint64_t o = __shfl_xor(v, d, 64); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ uint64_t dn_wave_max(uint64_t v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) { const uint64_t o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ uint64_t dn_wave_sum(uint64_t v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ uint64_t dn_wave_or(uint64_t v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v |= __shfl_xor(v, d, 64);
    return v;
}

// The census of one column by one workgroup of THREADS threads, tiles of THREADS * LOADS * 2 rows strided over the grid.
// census[] arrives as {~0, 0, 0, 0, 0, 0}.
template <int DT, int THREADS, int LOADS>
__device__ __forceinline__ void dn_census(const DnCol &c, unsigned long long *census) {
    constexpr int TILE = THREADS * LOADS * 2;
    const bool aligned = (reinterpret_cast<uintptr_t>(c.data) & 15) == 0;
    const int64_t tiles = (c.n + TILE - 1) / TILE;
    uint64_t mn = ~0ull, mx = 0, n_nan = 0, n_null = 0, n_valid = 0, flags = 0;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t r0 = t * TILE + 2 * (int64_t)threadIdx.x;
        uint64_t v[LOADS][2];
        uint32_t in[LOADS], nul[LOADS];
#pragma unroll
        for (int k = 0; k < LOADS; k++) {
            const int64_t r = r0 + (int64_t)k * 2 * THREADS;
            dn_load2<DT>(c, r, aligned, v[k], in[k]);
            nul[k] = c.null && in[k] ? ((uint32_t)c.null[r >> 3] >> (r & 7)) & 3 : 0;
        }
#pragma unroll
        for (int k = 0; k < LOADS; k++)
#pragma unroll
            for (int j = 0; j < 2; j++) {
                if (!((in[k] >> j) & 1)) continue;
                if ((nul[k] >> j) & 1) { n_null++; continue; }
                const uint64_t b = v[k][j];
                if (DT == PANDRS_HIP_F64) {
                    if (dn_is_nan(b)) { n_nan++; continue; }
                    const double x = __longlong_as_double((long long)b);
                    if (!(fabs(x) <= 9007199254740992.0) || x != trunc(x)) flags |= DN_F_FRACTION;
                    if (b == 0x8000000000000000ull) flags |= DN_F_NEGZERO;
                }
                const uint64_t im = dn_image<DT>(b);
                mn = im < mn ? im : mn;
                mx = im > mx ? im : mx;
                n_valid++;
            }
    }
    mn = dn_wave_min(mn); mx = dn_wave_max(mx);
    n_nan = dn_wave_sum(n_nan); n_null = dn_wave_sum(n_null); n_valid = dn_wave_sum(n_valid); flags = dn_wave_or(flags);
    if ((threadIdx.x & 63) == 0) {
        if (n_valid) { atomicMin(&census[DN_MIN], (unsigned long long)mn); atomicMax(&census[DN_MAX], (unsigned long long)mx); }
        if (n_nan) atomicAdd(&census[DN_NAN], (unsigned long long)n_nan);
        if (n_null) atomicAdd(&census[DN_NULL], (unsigned long long)n_null);
        if (n_valid) atomicAdd(&census[DN_VALID], (unsigned long long)n_valid);
        if (flags) atomicOr(&census[DN_FLAGS], (unsigned long long)flags);
    }
}

// The table index of a number: its distance from the smallest one.  I64 in wrapping unsigned arithmetic (I64_MIN .. I64_MAX
// does not overflow), F64 (integral, |v| <= 2^53: the conversion is exact) through int64.
template <int DT>
__device__ __forceinline__ uint64_t dn_cell_index(uint64_t cell, uint64_t base) {
    if (DT == PANDRS_HIP_F64) return (uint64_t)(int64_t)__longlong_as_double((long long)cell) - base;
    return cell - base;
}

struct DnRank {
    const uint32_t *rank;     // the string pool's rank table, or nullptr: by code
    uint64_t n_codes;
};

// what an entry sorts by in the value order: ascending int64
template <int DT>
__device__ __forceinline__ int64_t dn_order_key(uint64_t cell, const DnRank &rk) {
    if (DT == PANDRS_HIP_U32CODE && rk.rank) return cell < rk.n_codes ? (int64_t)rk.rank[cell] : (int64_t)cell;
    return (int64_t)(dn_image<DT>(cell) ^ (DT == PANDRS_HIP_I64 || DT == PANDRS_HIP_F64 ? 0x8000000000000000ull : 0ull));
}

// Host side of the census: the numbers' span as a table.  *base = the smallest number as the table counts it, *span = max - min in
// unsigned 64-bit (cells = span + 1 may be 2^64; no number at all: a table of one empty cell).  false: an F64 column that is
// not addressable by value (a fraction, a number beyond +-2^53 or a -0.0).
inline bool dn_span(int dt, const uint64_t cs[DN_CENSUS_WORDS], uint64_t *base, uint64_t *span) {
    *base = 0; *span = 0;
    if (!cs[DN_VALID]) return true;
    if (dt == PANDRS_HIP_I64) { *base = cs[DN_MIN] ^ 0x8000000000000000ull; *span = cs[DN_MAX] - cs[DN_MIN]; return true; }
    if (dt == PANDRS_HIP_F64) {
        *span = ~0ull;
        if (cs[DN_FLAGS] & (DN_F_FRACTION | DN_F_NEGZERO)) return false;
        auto dec = [](uint64_t e) { const uint64_t b = (e >> 63) ? (e & 0x7FFFFFFFFFFFFFFFull) : ~e; double d; std::memcpy(&d, &b, 8); return d; };
        const int64_t lo = (int64_t)dec(cs[DN_MIN]), hi = (int64_t)dec(cs[DN_MAX]);      // |v| <= 2^53: exact
        *base = (uint64_t)lo;
        *span = (uint64_t)hi - (uint64_t)lo;
        return true;
    }
    *base = cs[DN_MIN]; *span = cs[DN_MAX] - cs[DN_MIN];
    return true;
}

#define DN_DISPATCH(dtype, CALL)                                        \
    switch (dtype) {                                                    \
    case PANDRS_HIP_I64: { constexpr int DT = PANDRS_HIP_I64; CALL; break; }          \
    case PANDRS_HIP_F64: { constexpr int DT = PANDRS_HIP_F64; CALL; break; }          \
    case PANDRS_HIP_U32CODE: { constexpr int DT = PANDRS_HIP_U32CODE; CALL; break; }  \
    default: { constexpr int DT = PANDRS_HIP_BOOLBITS; CALL; break; }   \
    }

}  // namespace pandrs
