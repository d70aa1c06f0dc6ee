// The pools of the FID Inception-v3 on gfx950 (stylegan2/inception.py): the three 3x3 windows the network uses and its final
// global average.
//
//   IDEAS_POOL_MAX_S2          F.max_pool2d(x, 3, 2)                               OH = (H - 3) / 2 + 1, no padding
//   IDEAS_POOL_MAX_S1P1        F.max_pool2d(x, 3, 1, 1)                            OH = H; padding never wins
//   IDEAS_POOL_AVG_S1P1_VALID  F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)   OH = H; divisor = the in-image taps (4 / 6 / 9)
//   global average             adaptive_avg_pool2d(x, 1) -> float [B][C]
//
// Tensors are channels-innermost [B, H, W, C] in f32 or bf16, arithmetic is f32, one rounding at the store; channel vectors of VW
// elements by the rule of stream.hpp.
//
// Work split of the 3x3 windows: a thread owns one channel vector of a run of SEG consecutive outputs of one output row and walks
// along it with the COLUMN reductions of the window in registers: col[ix] = the reduction of the (up to) three rows of input
// column ix, out[ow] = the reduction of three columns.  A column is loaded once per run and used by every window of the run that
// covers it: 3 (SEG + 2) / SEG loads per output at stride 1 and 3 (2 SEG + 1) / SEG at stride 2 instead of 9; consecutive lanes
// take consecutive vectors of the same pixel, so every load and store of a wave is one contiguous run of memory.
//
// Max: torch's update rule (a greater value or a NaN replaces the running maximum), so a NaN anywhere in the window is the result;
// a missing (padding) tap is skipped, its stand-in -inf can never win against a tap of the image.  Average: the sum is
// (r0 + r1) + r2 down a column and then (c0 + c1) + c2 across the columns, missing taps contributing an exact +0, divided by the
// count of in-image taps: a fixed order that does not depend on how the row is cut into runs, so the result is bitwise reproducible.
// The global average adds the H W pixels of a channel in index order in one thread.  No atomics anywhere.
#include "stream.hpp"

namespace {

constexpr int P3_SEG_S1 = 8;          // outputs per thread, stride 1: 30 column loads for 8 outputs
constexpr int P3_SEG_S2 = 4;          // stride 2: 27 column loads for 4 outputs

struct Pool3Args {
    int B, H, W, C, OH, OW, L, NSEG;       // L = C / VW vectors per pixel, NSEG = runs per output row
};

__device__ __forceinline__ bool pool3_takes(float v, float m) { return v > m || v != v; }

// the reduction of input column ix over the rows iy0 .. iy0 + 2 that lie inside the image (ix itself is inside)
template <typename T, int VW, bool AVG>
__device__ __forceinline__ void pool3_column(const T* __restrict__ xb, const Pool3Args& a, int iy0, int ix, int v, float (&col)[VW]) {
#pragma unroll
    for (int e = 0; e < VW; ++e) col[e] = AVG ? 0.f : -INFINITY;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int iy = iy0 + r;
        if (iy < 0 || iy >= a.H) continue;
        float q[VW];
        chan_io<T, VW>::load(xb + ((int64_t)iy * a.W + ix) * a.C + (int64_t)v * VW, q);
#pragma unroll
        for (int e = 0; e < VW; ++e) {
            if (AVG) col[e] = col[e] + q[e];
            else if (pool3_takes(q[e], col[e])) col[e] = q[e];
        }
    }
}

template <int VW, bool AVG>
__device__ __forceinline__ void pool3_empty(float (&col)[VW]) {
#pragma unroll
    for (int e = 0; e < VW; ++e) col[e] = AVG ? 0.f : -INFINITY;
}

// S = stride (2: no padding, 1: one pixel of padding); AVG only with S = 1
template <typename T, int VW, int S, bool AVG>
__global__ __launch_bounds__(256) void pool3x3_kernel(T* __restrict__ y, const T* __restrict__ x, Pool3Args a) {
    constexpr int SEG = S == 2 ? P3_SEG_S2 : P3_SEG_S1;
    constexpr int P = S == 2 ? 0 : 1;
    const int64_t n = (int64_t)a.B * a.OH * a.NSEG * a.L;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int v = (int)(i % a.L);
        int64_t r = i / a.L;
        const int seg = (int)(r % a.NSEG);
        r /= a.NSEG;
        const int oh = (int)(r % a.OH);
        const int64_t b = r / a.OH;
        const T* xb = x + b * a.H * a.W * a.C;
        T* yrow = y + ((b * a.OH + oh) * a.OW) * a.C + (int64_t)v * VW;
        const int iy0 = oh * S - P;
        const int ow0 = seg * SEG;
        const int ow1 = ow0 + SEG < a.OW ? ow0 + SEG : a.OW;
        int rows = 3;                                   // in-image rows of the window (the average's divisor)
        if (iy0 < 0) --rows;
        if (iy0 + 2 >= a.H) --rows;
        float c0[VW], c1[VW], c2[VW], o[VW];
        if constexpr (S == 1) {
            // c0 = column ow - 1, c1 = column ow, c2 = column ow + 1
            if (ow0 - 1 >= 0) pool3_column<T, VW, AVG>(xb, a, iy0, ow0 - 1, v, c0); else pool3_empty<VW, AVG>(c0);
            pool3_column<T, VW, AVG>(xb, a, iy0, ow0, v, c1);
            for (int ow = ow0; ow < ow1; ++ow) {
                const bool right = ow + 1 < a.W;
                if (right) pool3_column<T, VW, AVG>(xb, a, iy0, ow + 1, v, c2); else pool3_empty<VW, AVG>(c2);
                if (AVG) {
                    const float cnt = (float)(rows * (1 + (ow > 0 ? 1 : 0) + (right ? 1 : 0)));
#pragma unroll
                    for (int e = 0; e < VW; ++e) o[e] = ((c0[e] + c1[e]) + c2[e]) / cnt;
                } else {
#pragma unroll
                    for (int e = 0; e < VW; ++e) {
                        float m = c0[e];
                        if (pool3_takes(c1[e], m)) m = c1[e];
                        if (pool3_takes(c2[e], m)) m = c2[e];
                        o[e] = m;
                    }
                }
                chan_io<T, VW>::store(yrow + (int64_t)ow * a.C, o);
#pragma unroll
                for (int e = 0; e < VW; ++e) { c0[e] = c1[e]; c1[e] = c2[e]; }
            }
        } else {
            // columns 2 ow, 2 ow + 1, 2 ow + 2, all inside the image (2 (OW - 1) + 2 <= W - 1); the last one is the next window's first
            pool3_column<T, VW, false>(xb, a, iy0, 2 * ow0, v, c0);
            for (int ow = ow0; ow < ow1; ++ow) {
                pool3_column<T, VW, false>(xb, a, iy0, 2 * ow + 1, v, c1);
                pool3_column<T, VW, false>(xb, a, iy0, 2 * ow + 2, v, c2);
#pragma unroll
                for (int e = 0; e < VW; ++e) {
                    float m = c0[e];
                    if (pool3_takes(c1[e], m)) m = c1[e];
                    if (pool3_takes(c2[e], m)) m = c2[e];
                    o[e] = m;
                }
                chan_io<T, VW>::store(yrow + (int64_t)ow * a.C, o);
#pragma unroll
                for (int e = 0; e < VW; ++e) c0[e] = c2[e];
            }
        }
    }
}

// one thread per (sample, channel vector): the H W pixels in index order, four loads in flight
template <typename T, int VW>
__global__ __launch_bounds__(256) void global_avg_kernel(float* __restrict__ out, const T* __restrict__ x, int B, int C, int HW, int L) {
    const int64_t n = (int64_t)B * L;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int v = (int)(i % L);
        const int64_t b = i / L;
        const T* p = x + b * HW * C + (int64_t)v * VW;
        float s[VW];
#pragma unroll
        for (int e = 0; e < VW; ++e) s[e] = 0.f;
        int q = 0;
        for (; q + 4 <= HW; q += 4) {
            float t[4][VW];
#pragma unroll
            for (int k = 0; k < 4; ++k) chan_io<T, VW>::load(p + (int64_t)(q + k) * C, t[k]);
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int e = 0; e < VW; ++e) s[e] = s[e] + t[k][e];
        }
        for (; q < HW; ++q) {
            float t[VW];
            chan_io<T, VW>::load(p + (int64_t)q * C, t);
#pragma unroll
            for (int e = 0; e < VW; ++e) s[e] = s[e] + t[e];
        }
        float* o = out + b * C + (int64_t)v * VW;
        const float cnt = (float)HW;
        if constexpr (VW == 1) {
            o[0] = s[0] / cnt;
        } else {
#pragma unroll
            for (int e = 0; e < VW; e += 4)
                *reinterpret_cast<float4*>(o + e) = make_float4(s[e] / cnt, s[e + 1] / cnt, s[e + 2] / cnt, s[e + 3] / cnt);
        }
    }
}

unsigned pool3_grid(int64_t n) {
    int64_t g = ideas_cdiv(n, 256);
    if (g > 65536) g = 65536;
    if (g < 1) g = 1;
    return (unsigned)g;
}

}  // namespace

extern "C" int ideas_pool3x3_fwd(void* y, const void* x, int B, int C, int H, int W, int mode, int dtype, void* stream_) {
    if (dtype != IDEAS_F32 && dtype != IDEAS_BF16) return IDEAS_E_UNSUPPORTED;
    if (mode != IDEAS_POOL_MAX_S2 && mode != IDEAS_POOL_MAX_S1P1 && mode != IDEAS_POOL_AVG_S1P1_VALID) return IDEAS_E_UNSUPPORTED;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return IDEAS_E_SHAPE;
    if (mode == IDEAS_POOL_MAX_S2 && (H < 3 || W < 3)) return IDEAS_E_SHAPE;                // no window fits
    if ((int64_t)H * W * C >= 0x7fffffffLL) return IDEAS_E_SHAPE;
    if (!y || !x) return IDEAS_E_NULL;
    const int s2 = mode == IDEAS_POOL_MAX_S2;
    const int vw = ideas_chan_vw(dtype, C, ideas_aligned16(y) && ideas_aligned16(x));
    Pool3Args a;
    a.B = B; a.H = H; a.W = W; a.C = C;
    a.OH = s2 ? (H - 3) / 2 + 1 : H;
    a.OW = s2 ? (W - 3) / 2 + 1 : W;
    a.L = C / vw;
    a.NSEG = (int)ideas_cdiv(a.OW, s2 ? P3_SEG_S2 : P3_SEG_S1);
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid(pool3_grid((int64_t)B * a.OH * a.NSEG * a.L));
    with_chan(dtype, vw, [&](auto c) {
        using T = typename decltype(c)::type;
        auto* kernel = mode == IDEAS_POOL_MAX_S2     ? pool3x3_kernel<T, c.VW, 2, false>
                       : mode == IDEAS_POOL_MAX_S1P1 ? pool3x3_kernel<T, c.VW, 1, false>
                                                     : pool3x3_kernel<T, c.VW, 1, true>;
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, (T*)y, (const T*)x, a);
    });
    return ideas_launch_status();
}

extern "C" int ideas_global_avg_pool(float* out, const void* x, int B, int C, int H, int W, int dtype, void* stream_) {
    if (dtype != IDEAS_F32 && dtype != IDEAS_BF16) return IDEAS_E_UNSUPPORTED;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return IDEAS_E_SHAPE;
    if ((int64_t)H * W >= 0x7fffffffLL / C) return IDEAS_E_SHAPE;
    if (!out || !x) return IDEAS_E_NULL;
    const int vw = ideas_chan_vw(dtype, C, ideas_aligned16(out) && ideas_aligned16(x));
    const int L = C / vw;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid(pool3_grid((int64_t)B * L));
    with_chan(dtype, vw, [&](auto c) {
        using T = typename decltype(c)::type;
        hipLaunchKernelGGL((global_avg_kernel<T, c.VW>), grid, dim3(256), 0, stream, out, (const T*)x, B, C, H * W, L);
    });
    return ideas_launch_status();
}
