// describe.hpp — what describe.hip (moments, radix select, order statistics) and moments.hip (fused sums of many columns) share:
// the column view, the cell decoders, the stream whose fold order depends on row numbers only, and the workgroup sum.
#pragma once
#include "engine.hpp"

namespace pandrs {

constexpr int DS_THREADS = 256;
constexpr int DS_LOADS = 4;                              // 16-byte loads in flight per thread
constexpr int DS_TILE = DS_THREADS * DS_LOADS * 2;       // rows per workgroup iteration (2048; pandrs_hip.h: describe_tile_rows)
constexpr int DS_BLOCKS_PER_CU = 4;                      // grid = min(4 x CUs, tiles): what the digit stream's 33 KB of LDS keeps
                                                         // resident per CU, so no launch runs in two rounds (pandrs_hip.h)

struct DsCol {
    const uint64_t *data;     // 8-byte aligned
    const uint8_t *null;      // LSB-first, 1 = null, any byte offset
    int64_t n;
    int i64;
};

__device__ __forceinline__ bool ds_is_nan(uint64_t b, int i64) { return !i64 && (b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull; }
__device__ __forceinline__ double ds_value(uint64_t b, int i64) { return i64 ? (double)(int64_t)b : __longlong_as_double((long long)b); }
__device__ __forceinline__ uint64_t ds_code(uint64_t b, int i64) { return i64 ? enc_i64((int64_t)b) : enc_f64(__longlong_as_double((long long)b)); }
__device__ __forceinline__ double ds_decode(uint64_t code, int i64) { return i64 ? (double)dec_i64(code) : dec_f64(code); }

// f(bits, valid) for every row, called by all threads of the workgroup together (f may ballot).  A thread's rows depend on
// the row numbers only, never on the address, so every floating-point fold has one order and a column gives the same bits
// wherever it lies.  A data pointer that is 8 bytes off a 16-byte boundary takes its row pairs as two 8-byte loads.
template <class F>
__device__ __forceinline__ void ds_stream(const DsCol &c, F &&f) {
    const bool aligned = (reinterpret_cast<uintptr_t>(c.data) & 15) == 0;
    const int64_t tiles = (c.n + DS_TILE - 1) / DS_TILE;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t r0 = t * DS_TILE + 2 * (int64_t)threadIdx.x;
        uint64_t v[DS_LOADS][2];
        uint32_t ok[DS_LOADS];
#pragma unroll
        for (int k = 0; k < DS_LOADS; k++) {
            const int64_t r = r0 + (int64_t)k * 2 * DS_THREADS;          // even: both rows' mask bits lie in one byte
            uint32_t in = 0;
            v[k][0] = v[k][1] = 0;
            if (r + 1 < c.n) {
                if (aligned) {
                    const ulonglong2 q = *reinterpret_cast<const ulonglong2 *>(c.data + r);
                    v[k][0] = q.x; v[k][1] = q.y;
                } else {
                    v[k][0] = c.data[r]; v[k][1] = c.data[r + 1];
                }
                in = 3;
            } else if (r < c.n) {
                v[k][0] = c.data[r];
                in = 1;
            }
            if (c.null && in) in &= ~((uint32_t)c.null[r >> 3] >> (r & 7));
            ok[k] = in;
        }
#pragma unroll
        for (int k = 0; k < DS_LOADS; k++) {
            f(v[k][0], (ok[k] & 1) != 0);
            f(v[k][1], (ok[k] & 2) != 0);
        }
    }
}

__device__ __forceinline__ double ds_block_sum(double v, double *sh) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = sh[0];
    for (int w = 1; w < DS_THREADS / 64; w++) r += sh[w];
    __syncthreads();
    return r;
}

// the same fold for a count
__device__ __forceinline__ uint64_t ds_block_count(uint64_t v, uint64_t *sh) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t r = sh[0];
    for (int w = 1; w < DS_THREADS / 64; w++) r += sh[w];
    __syncthreads();
    return r;
}

}  // namespace pandrs
