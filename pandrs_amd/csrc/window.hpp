// window.hpp — the column view and the window bounds shared by window.hip (the fold, van Herk and scan statistics) and
// window_quantile.hip (the order statistics).
#pragma once
#include "engine.hpp"

namespace pandrs {

constexpr int WN_THREADS = 256;

// ---- the column and the window bounds ------------------------------------------------------------------------------------
struct WnCol {
    const void *data;
    const uint8_t *null;      // LSB-first, 1 = null, any byte offset
    int64_t n, nbytes;
    int i64;
    __device__ __forceinline__ double x(int64_t r) const {
        return i64 ? (double)static_cast<const int64_t *>(data)[r] : static_cast<const double *>(data)[r];
    }
    __device__ __forceinline__ bool valid(int64_t r) const { return !null || !((null[r >> 3] >> (r & 7)) & 1); }
    __device__ __forceinline__ uint64_t word(int64_t wi) const {          // null bits [64 wi, 64 wi + 64)
        const int64_t b = wi * 8;
        if (b + 8 <= nbytes && (reinterpret_cast<uintptr_t>(null) & 7) == 0) return *reinterpret_cast<const uint64_t *>(null + b);
        uint64_t v = 0;
        for (int k = 0; k < 8; k++)
            if (b + k < nbytes) v |= (uint64_t)null[b + k] << (8 * k);
        return v;
    }
    __device__ int64_t nulls_in(int64_t a, int64_t b) const {             // null rows in [a, b)
        if (!null || a >= b) return 0;
        const int64_t wa = a >> 6, wb = (b - 1) >> 6;
        int64_t c = 0;
        for (int64_t wi = wa; wi <= wb; wi++) {
            uint64_t m = word(wi);
            if (wi == wa) m &= ~0ull << (a & 63);
            if (wi == wb && (b & 63)) m &= (1ull << (b & 63)) - 1;
            c += __popcll(m);
        }
        return c;
    }
};

// series/window.rs:175-190: trailing [max(0, i+1-w), i+1); centred start = i >= w/2 ? i - w/2 : 0, end = min(start+w, n).
// w is clamped to 2n+2 by the host, which changes no window and keeps start + w in range.
struct WnGeom {
    int64_t n, w, half;
    int center;
    __device__ __forceinline__ void bounds(int64_t i, int64_t &s, int64_t &e) const {
        if (center) {
            s = i >= half ? i - half : 0;
            e = s + w < n ? s + w : n;
        } else {
            s = i + 1 >= w ? i + 1 - w : 0;
            e = i + 1;
        }
    }
};

}  // namespace pandrs
