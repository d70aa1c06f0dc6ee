// The scan of a baseline JPEG file, as its writer (jpeg_bytes.hip) and its reader (jpeg_decode.hip) both walk it: the zigzag order, the
// MCU geometry with the dummy luma blocks of 4:2:0, and the workgroup prefix sum both use to turn counts into offsets.  The stream is
// stated in include/ideas_hip.h ("The JPEG file, written").
#pragma once
#include "common.hpp"

namespace {

// natural index 8 u + v of zigzag position k
__device__ const unsigned char k_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// The scan of one image: MCUs in raster order, in each the hs x hs luma blocks in raster order, then Cb, then Cr.
struct scan_geom {
    int C, hs, per_mcu;            // per_mcu = hs * hs + (C == 3 ? 2 : 0) blocks
    int mw;                        // MCU columns
    int bhn, bwn;                  // the luma block grid of coef_y
    int64_t nmcu, nblk;            // MCUs (= the chroma block grid of coef_c) and blocks of one image
};

// host side: the geometry of a C x H x W image at this subsampling (arguments already checked)
inline scan_geom make_scan_geom(int C, int H, int W, int sub) {
    scan_geom g;
    g.C = C;
    g.hs = C == 3 && sub == 2 ? 2 : 1;
    g.per_mcu = g.hs * g.hs + (C == 3 ? 2 : 0);
    g.mw = (int)ideas_cdiv(W, 8 * g.hs);
    g.bhn = (int)ideas_cdiv(H, 8);
    g.bwn = (int)ideas_cdiv(W, 8);
    g.nmcu = ideas_cdiv(H, 8 * g.hs) * g.mw;
    g.nblk = g.nmcu * g.per_mcu;
    return g;
}

// The luma block (by, bx) of coef_y whose DC scan block `slot` of MCU (my, mx) carries: the block itself where it exists.  A block right
// of the grid is a dummy with the DC of the block on its left; a block below it one with the DC of slot (0, 1), itself a dummy where
// the grid is short on the right too.  Slot 0 always exists.
__device__ __forceinline__ bool luma_source(const scan_geom& g, int my, int mx, int slot, int& by, int& bx) {
    by = my * g.hs + (g.hs == 2 ? slot >> 1 : 0);
    bx = mx * g.hs + (g.hs == 2 ? slot & 1 : 0);
    const bool real = by < g.bhn && bx < g.bwn;
    if (by >= g.bhn) {
        by = my * 2;
        bx = min(mx * 2 + 1, g.bwn - 1);
    } else if (bx >= g.bwn) {
        bx -= 1;
    }
    return real;
}

// Exclusive prefix sum of one value a thread over the workgroup of 256; total = the sum.  s_w: 4 words of LDS.  Two barriers; the
// first one also ends the previous call's reads of s_w.
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned* s_w, unsigned& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    unsigned before = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        before += i < wave ? s_w[i] : 0u;
        total += s_w[i];
    }
    return before + inc - v;
}

}  // namespace
