// The two image transforms of adaptive discriminator augmentation (stylegan2/non_leaking.py:316-391), for gfx950.
//
//   affine warp     y[b,c,oy,ox] = the bilinear blend of the four pixels of x[b,c] around
//                       (sx, sy) = (t0*ox + t1*oy + t2, t3*ox + t4*oy + t5),     t = theta[b] (six floats a sample)
//                   a tap outside [0,W-1] x [0,H-1] contributes zero: F.grid_sample(mode="bilinear", padding_mode="zeros") with the
//                   grid's affine map, the 1/size rescale and the un-normalisation folded into theta on the host.  The reference
//                   builds an [N,h,w,3] grid, multiplies it by the matrix, rescales it and samples: three full-size grid tensors.
//   its adjoint     gx[b,c,iy,ix] += w * gy[b,c,oy,ox] over the same taps and weights (warp_taps is the ONE expression of both).
//                   Several output pixels land on one input pixel, so the sums are f32 atomics: the order of summation is not
//                   fixed, as in ideas_patch_resize_bwd and in torch's own grid_sample backward.
//   colour affine   y[b,i,p] = m[b][4i]*x[b,0,p] + m[b][4i+1]*x[b,1,p] + m[b][4i+2]*x[b,2,p] + m[b][4i+3]  (C = 3), one pass; the
//                   reference runs permute, batched matmul, add, permute.  Its adjoint is the same call with the transposed 3x3
//                   and a zero last column.
//
// f32 or bf16 tensors (f32 arithmetic, one rounding at the store), NCHW or NHWC.
//
// Work split.  NCHW: one thread per output pixel, looping over c -- the taps and weights are computed once a pixel and a wave
// stores 64 consecutive elements of a plane.  NHWC: one thread per (pixel, channel vector of VW elements by the rule of
// stream.hpp).  Consecutive threads take consecutive addresses of y in every case.
//
// Out-of-range safety.  A position is used only if it lies in (-1, W) x (-1, H) -- a comparison that is false for NaN -- and
// the sample's six theta values are all finite; otherwise the four weights are zero.  The tap indices are clamped into the image
// BEFORE any address is formed, whatever theta holds.
#include "stream.hpp"

namespace {

struct WarpTaps {
    int x0, x1, y0, y1;              // clamped into [0,W-1] / [0,H-1]
    float w00, w01, w10, w11;        // w[yi][xi]; zero for a tap outside the image
};

__device__ __forceinline__ WarpTaps warp_taps(const float* __restrict__ th, int ox, int oy, int H, int W) {
    const float t0 = th[0], t1 = th[1], t2 = th[2], t3 = th[3], t4 = th[4], t5 = th[5];
    const float fx = (float)ox, fy = (float)oy;
    const float sx = fmaf(t0, fx, fmaf(t1, fy, t2));
    const float sy = fmaf(t3, fx, fmaf(t4, fy, t5));
    const bool finite = isfinite(t0) && isfinite(t1) && isfinite(t2) && isfinite(t3) && isfinite(t4) && isfinite(t5);
    const bool inside = finite && sx > -1.f && sx < (float)W && sy > -1.f && sy < (float)H;
    WarpTaps t;
    // (inside: floorf(sx) is in [-1, W-1], so the conversion cannot overflow; outside the position is replaced by 0)
    const float px = inside ? sx : 0.f, py = inside ? sy : 0.f;
    const float flx = floorf(px), fly = floorf(py);
    const int ix = (int)flx, iy = (int)fly;
    const float ax = px - flx, ay = py - fly;                      // exact
    const float wx0 = (inside && ix >= 0) ? 1.f - ax : 0.f;
    const float wx1 = (inside && ix + 1 <= W - 1) ? ax : 0.f;
    const float wy0 = (inside && iy >= 0) ? 1.f - ay : 0.f;
    const float wy1 = (inside && iy + 1 <= H - 1) ? ay : 0.f;
    t.x0 = min(max(ix, 0), W - 1);
    t.x1 = min(max(ix + 1, 0), W - 1);
    t.y0 = min(max(iy, 0), H - 1);
    t.y1 = min(max(iy + 1, 0), H - 1);
    t.w00 = wy0 * wx0; t.w01 = wy0 * wx1; t.w10 = wy1 * wx0; t.w11 = wy1 * wx1;
    return t;
}

__device__ __forceinline__ float warp_blend(const WarpTaps& t, float a, float b, float c, float d) {
    return t.w00 * a + t.w01 * b + t.w10 * c + t.w11 * d;
}

struct WarpArgs {
    int B, C, H, W, OH, OW;
    int L;                 // NHWC: vectors (or elements) of a pixel
    int64_t n;             // threads that have work
};

// the thread's output pixel: i -> (b, oy, ox)
__device__ __forceinline__ void warp_pixel(int64_t pix, const WarpArgs& a, int& b, int& oy, int& ox) {
    ox = (int)(pix % a.OW);
    const int64_t r = pix / a.OW;
    oy = (int)(r % a.OH);
    b = (int)(r / a.OH);
}

// ---- NCHW: one thread per output pixel ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void warp_nchw_kernel(T* __restrict__ y, const T* __restrict__ x, const float* __restrict__ theta,
                                                        WarpArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    int b, oy, ox;
    warp_pixel(i, a, b, oy, ox);
    const WarpTaps t = warp_taps(theta + (int64_t)b * 6, ox, oy, a.H, a.W);
    const int64_t ip = (int64_t)a.H * a.W, op = (int64_t)a.OH * a.OW;
    const int64_t o00 = (int64_t)t.y0 * a.W + t.x0, o01 = (int64_t)t.y0 * a.W + t.x1;
    const int64_t o10 = (int64_t)t.y1 * a.W + t.x0, o11 = (int64_t)t.y1 * a.W + t.x1;
    const T* xp = x + (int64_t)b * a.C * ip;
    T* yp = y + (int64_t)b * a.C * op + (int64_t)oy * a.OW + ox;
    for (int c = 0; c < a.C; ++c, xp += ip, yp += op)
        st1(yp, warp_blend(t, ld1(xp + o00), ld1(xp + o01), ld1(xp + o10), ld1(xp + o11)));
}

template <typename T>
__global__ __launch_bounds__(256) void warp_bwd_nchw_kernel(float* __restrict__ gx, const T* __restrict__ gy,
                                                            const float* __restrict__ theta, WarpArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    int b, oy, ox;
    warp_pixel(i, a, b, oy, ox);
    const WarpTaps t = warp_taps(theta + (int64_t)b * 6, ox, oy, a.H, a.W);
    const int64_t ip = (int64_t)a.H * a.W, op = (int64_t)a.OH * a.OW;
    const int64_t o00 = (int64_t)t.y0 * a.W + t.x0, o01 = (int64_t)t.y0 * a.W + t.x1;
    const int64_t o10 = (int64_t)t.y1 * a.W + t.x0, o11 = (int64_t)t.y1 * a.W + t.x1;
    float* gp = gx + (int64_t)b * a.C * ip;
    const T* yp = gy + (int64_t)b * a.C * op + (int64_t)oy * a.OW + ox;
    for (int c = 0; c < a.C; ++c, gp += ip, yp += op) {
        const float g = ld1(yp);
        if (t.w00 != 0.f) atomicAdd(gp + o00, t.w00 * g);
        if (t.w01 != 0.f) atomicAdd(gp + o01, t.w01 * g);
        if (t.w10 != 0.f) atomicAdd(gp + o10, t.w10 * g);
        if (t.w11 != 0.f) atomicAdd(gp + o11, t.w11 * g);
    }
}

// ---- NHWC: one thread per (output pixel, vector of VW channels) -----------------------------------------------------------------
template <typename T, int VW>
__global__ __launch_bounds__(256) void warp_nhwc_kernel(T* __restrict__ y, const T* __restrict__ x, const float* __restrict__ theta,
                                                        WarpArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const int v = (int)(i % a.L);
    int b, oy, ox;
    warp_pixel(i / a.L, a, b, oy, ox);
    const WarpTaps t = warp_taps(theta + (int64_t)b * 6, ox, oy, a.H, a.W);
    const T* xp = x + (int64_t)b * a.H * a.W * a.C + (int64_t)v * VW;
    float p00[VW], p01[VW], p10[VW], p11[VW], o[VW];
    chan_io<T, VW>::load(xp + ((int64_t)t.y0 * a.W + t.x0) * a.C, p00);
    chan_io<T, VW>::load(xp + ((int64_t)t.y0 * a.W + t.x1) * a.C, p01);
    chan_io<T, VW>::load(xp + ((int64_t)t.y1 * a.W + t.x0) * a.C, p10);
    chan_io<T, VW>::load(xp + ((int64_t)t.y1 * a.W + t.x1) * a.C, p11);
#pragma unroll
    for (int e = 0; e < VW; ++e) o[e] = warp_blend(t, p00[e], p01[e], p10[e], p11[e]);
    chan_io<T, VW>::store(y + i * VW, o);            // (pixel * L + v) * VW = pixel * C + v * VW
}

template <typename T, int VW>
__global__ __launch_bounds__(256) void warp_bwd_nhwc_kernel(float* __restrict__ gx, const T* __restrict__ gy,
                                                            const float* __restrict__ theta, WarpArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const int v = (int)(i % a.L);
    int b, oy, ox;
    warp_pixel(i / a.L, a, b, oy, ox);
    const WarpTaps t = warp_taps(theta + (int64_t)b * 6, ox, oy, a.H, a.W);
    float* gp = gx + (int64_t)b * a.H * a.W * a.C + (int64_t)v * VW;
    float g[VW];
    chan_io<T, VW>::load(gy + i * VW, g);
    float* q00 = gp + ((int64_t)t.y0 * a.W + t.x0) * a.C;
    float* q01 = gp + ((int64_t)t.y0 * a.W + t.x1) * a.C;
    float* q10 = gp + ((int64_t)t.y1 * a.W + t.x0) * a.C;
    float* q11 = gp + ((int64_t)t.y1 * a.W + t.x1) * a.C;
#pragma unroll
    for (int e = 0; e < VW; ++e) {
        if (t.w00 != 0.f) atomicAdd(q00 + e, t.w00 * g[e]);
        if (t.w01 != 0.f) atomicAdd(q01 + e, t.w01 * g[e]);
        if (t.w10 != 0.f) atomicAdd(q10 + e, t.w10 * g[e]);
        if (t.w11 != 0.f) atomicAdd(q11 + e, t.w11 * g[e]);
    }
}

// ---- colour affine: one thread per pixel ----------------------------------------------------------------------------------------
template <typename T, bool NHWC>
__global__ __launch_bounds__(256) void color_affine_kernel(T* __restrict__ y, const T* __restrict__ x, const float* __restrict__ m,
                                                           int64_t P, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t b = i / P, p = i - b * P;
    const float* mb = m + b * 12;
    const int64_t base = NHWC ? i * 3 : b * 3 * P + p;
    const int64_t cs = NHWC ? 1 : P;               // channel stride
    const float r = ld1(x + base), g = ld1(x + base + cs), bl = ld1(x + base + 2 * cs);
#pragma unroll
    for (int k = 0; k < 3; ++k)
        st1(y + base + k * cs, fmaf(mb[4 * k + 2], bl, fmaf(mb[4 * k + 1], g, fmaf(mb[4 * k], r, mb[4 * k + 3]))));
}

int warp_check(int B, int C, int H, int W, int OH, int OW, int layout, int dtype) {
    if (dtype != IDEAS_F32 && dtype != IDEAS_BF16) return IDEAS_E_UNSUPPORTED;
    if (layout != IDEAS_NCHW && layout != IDEAS_NHWC) return IDEAS_E_UNSUPPORTED;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0) return IDEAS_E_SHAPE;
    if ((int64_t)H * W > 0x7fffffffLL || (int64_t)OH * OW > 0x7fffffffLL) return IDEAS_E_SHAPE;
    return IDEAS_OK;
}

// geometry of a launch; vw: the channel vector of the NHWC kernels (1 on NCHW)
WarpArgs warp_args(int B, int C, int H, int W, int OH, int OW, int layout, int dtype, bool aligned, int* vw) {
    *vw = ideas_chan_vw(dtype, C, layout == IDEAS_NHWC && aligned);
    WarpArgs a;
    a.B = B; a.C = C; a.H = H; a.W = W; a.OH = OH; a.OW = OW;
    a.L = layout == IDEAS_NHWC ? C / *vw : 1;
    a.n = (int64_t)B * OH * OW * a.L;
    return a;
}

}  // namespace

extern "C" int ideas_affine_warp(void* y, const void* x, const float* theta, int B, int C, int H, int W, int OH, int OW, int layout,
                                 int dtype, void* stream_) {
    if (const int rc = warp_check(B, C, H, W, OH, OW, layout, dtype)) return rc;
    if (!y || !x || !theta) return IDEAS_E_NULL;
    int vw;
    const WarpArgs a = warp_args(B, C, H, W, OH, OW, layout, dtype, ideas_aligned16(y) && ideas_aligned16(x), &vw);
    const dim3 grid((unsigned)ideas_cdiv(a.n, 256)), block(256);
    hipStream_t s = (hipStream_t)stream_;
    with_chan(dtype, vw, [&](auto c) {
        using T = typename decltype(c)::type;
        auto* kernel = layout == IDEAS_NCHW ? warp_nchw_kernel<T> : warp_nhwc_kernel<T, c.VW>;
        hipLaunchKernelGGL(kernel, grid, block, 0, s, (T*)y, (const T*)x, theta, a);
    });
    return ideas_launch_status();
}

extern "C" int ideas_affine_warp_bwd(float* gx, const void* gy, const float* theta, int B, int C, int H, int W, int OH, int OW,
                                     int clear, int layout, int dtype, void* stream_) {
    if (const int rc = warp_check(B, C, H, W, OH, OW, layout, dtype)) return rc;
    if (!gx || !gy || !theta) return IDEAS_E_NULL;
    hipStream_t s = (hipStream_t)stream_;
    if (clear) {
        const hipError_t e = hipMemsetAsync(gx, 0, (size_t)B * C * H * W * sizeof(float), s);
        if (e != hipSuccess) return (int)e;
    }
    int vw;
    const WarpArgs a = warp_args(B, C, H, W, OH, OW, layout, dtype, ideas_aligned16(gy), &vw);
    const dim3 grid((unsigned)ideas_cdiv(a.n, 256)), block(256);
    with_chan(dtype, vw, [&](auto c) {
        using T = typename decltype(c)::type;
        auto* kernel = layout == IDEAS_NCHW ? warp_bwd_nchw_kernel<T> : warp_bwd_nhwc_kernel<T, c.VW>;
        hipLaunchKernelGGL(kernel, grid, block, 0, s, gx, (const T*)gy, theta, a);
    });
    return ideas_launch_status();
}

extern "C" int ideas_color_affine(void* y, const void* x, const float* m, int B, int H, int W, int layout, int dtype, void* stream_) {
    if (dtype != IDEAS_F32 && dtype != IDEAS_BF16) return IDEAS_E_UNSUPPORTED;
    if (layout != IDEAS_NCHW && layout != IDEAS_NHWC) return IDEAS_E_UNSUPPORTED;
    if (B <= 0 || H <= 0 || W <= 0 || (int64_t)H * W > 0x7fffffffLL) return IDEAS_E_SHAPE;
    if (!y || !x || !m) return IDEAS_E_NULL;
    const int64_t P = (int64_t)H * W, n = (int64_t)B * P;
    const dim3 grid((unsigned)ideas_cdiv(n, 256)), block(256);
    hipStream_t s = (hipStream_t)stream_;
    with_dtype(dtype, [&](auto c) {
        using T = typename decltype(c)::type;
        auto* kernel = layout == IDEAS_NHWC ? color_affine_kernel<T, true> : color_affine_kernel<T, false>;
        hipLaunchKernelGGL(kernel, grid, block, 0, s, (T*)y, (const T*)x, m, P, n);
    });
    return ideas_launch_status();
}
