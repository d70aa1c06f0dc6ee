// LPIPS (VGG) on gfx950: the 2x2 max pool of the backbone and the per-layer head of the learned perceptual distance
// (stylegan2/lpips/networks_basic.py:64-92 with spatial=False, lpips=True; normalize_tensor of lpips/__init__.py:42-44).
//
//   pool forward    y[b,oh,ow,c] = max of x[b, 2oh + {0,1}, 2ow + {0,1}, c]      OH = H / 2, OW = W / 2 (floor): an odd trailing row
//                                                                                or column belongs to no window
//   pool backward   gx = gy at the window's maximum, 0 elsewhere (trailing rows / columns included): every element written once
//                   by the thread that owns its window -- no memset, no atomics.  Ties: the first element in row-major order; a
//                   NaN is the maximum, a later NaN replaces an earlier one (the update rule of torch's max_pool2d).
//   head forward    n_i[p] = sqrt(sum_c f_i[p,c]^2);  u_i = f_i / (n_i + 1e-10);  d[b] = (1/(HW)) sum_p sum_c w[c] (u_0 - u_1)^2
//   head backward   g_c = 2 w_c (u_0c - u_1c) gd[b] / (HW)
//                   gf0_k =   g_k / (n_0 + eps) - f0_k (sum_c g_c f0_c) / (n_0 (n_0 + eps)^2)
//                   gf1_k = -(g_k / (n_1 + eps) - f1_k (sum_c g_c f1_c) / (n_1 (n_1 + eps)^2))
//                   A pixel with n_i = 0 gets gf_i = 0 (the reference's sqrt backward gives NaN there), see DESIGN.md 3.13.
//
// Tensors are channels-innermost [B, H, W, C] in f32 or bf16, arithmetic is f32 (the sum over pixels is double), one rounding at
// the store; w, gd and d are f32.  Channel vectors of VW elements by the rule of stream.hpp.
//
// Head work split: a pixel is owned by a group of G = ideas_lane_group(C / VW) lanes; lane l takes the vectors l, l + G, ... (at
// most KV of them, a template parameter) of BOTH tensors and keeps them in registers, so each tensor is read from HBM once: the
// two norms, then the weighted sum (the dot products in the backward), are group_sum butterflies.  Consecutive groups take
// consecutive pixels.
//
// d[b] without floating-point atomics: grid (nblk, B); lane 0 of a group adds its pixels in double in index order, block_sum_256
// gives ONE double per block and sample; a second small kernel adds the <= IDEAS_LPIPS_MAX_PARTIALS partials of a sample in index
// order and applies 1/(HW).  The backward has no reduction across pixels.  Everything here is bitwise reproducible.
#include "stream.hpp"

namespace {

constexpr int LP_MAX_BLOCKS = IDEAS_LPIPS_MAX_PARTIALS;
constexpr float LP_EPS = 1e-10f;
constexpr int LP_MAX_LANE_ELEMS = 32;                     // elements of one tensor a lane holds: C <= 64 * 32

// ---- 2x2 max pool ---------------------------------------------------------------------------------------------------------------
struct PoolArgs {
    int B, H, W, C, OH, OW, L;       // L = C / VW vectors per pixel
};

// torch's update rule (max_pool2d): a later element replaces the running maximum when it is greater, or a NaN
__device__ __forceinline__ bool pool_takes(float v, float m) { return v > m || v != v; }

template <typename T, int VW>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(T* __restrict__ y, const T* __restrict__ x, PoolArgs a) {
    const int64_t n = (int64_t)a.B * a.OH * a.OW * a.L;
    const int64_t row = (int64_t)a.W * a.C;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int v = (int)(i % a.L);
        int64_t r = i / a.L;
        const int ow = (int)(r % a.OW);
        r /= a.OW;
        const int oh = (int)(r % a.OH);
        const int64_t b = r / a.OH;
        // 2 oh + 1 < H and 2 ow + 1 < W: OH = H / 2, OW = W / 2
        const int64_t base = ((b * a.H + 2 * oh) * a.W + 2 * ow) * a.C + (int64_t)v * VW;
        float q[4][VW], m[VW];
        chan_io<T, VW>::load(x + base, q[0]);
        chan_io<T, VW>::load(x + base + a.C, q[1]);
        chan_io<T, VW>::load(x + base + row, q[2]);
        chan_io<T, VW>::load(x + base + row + a.C, q[3]);
#pragma unroll
        for (int e = 0; e < VW; ++e) {
            m[e] = q[0][e];
#pragma unroll
            for (int k = 1; k < 4; ++k)
                if (pool_takes(q[k][e], m[e])) m[e] = q[k][e];
        }
        chan_io<T, VW>::store(y + ((b * a.OH + oh) * a.OW + ow) * a.C + (int64_t)v * VW, m);
    }
}

// one thread per vector of a window of the grid ceil(H/2) x ceil(W/2): a whole window scatters gy to its maximum and zeroes its
// other three elements; a window cut by the trailing row / column zeroes what of it lies inside the tensor
template <typename T, int VW>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(T* __restrict__ gx, const T* __restrict__ gy, const T* __restrict__ x, PoolArgs a) {
    const int EH = (a.H + 1) / 2, EW = (a.W + 1) / 2;
    const int64_t n = (int64_t)a.B * EH * EW * a.L;
    const int64_t row = (int64_t)a.W * a.C;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int v = (int)(i % a.L);
        int64_t r = i / a.L;
        const int ew = (int)(r % EW);
        r /= EW;
        const int eh = (int)(r % EH);
        const int64_t b = r / EH;
        const int64_t base = ((b * a.H + 2 * eh) * a.W + 2 * ew) * a.C + (int64_t)v * VW;
        float o[4][VW];
        if (eh < a.OH && ew < a.OW) {
            float q[4][VW], g[VW];
            chan_io<T, VW>::load(x + base, q[0]);
            chan_io<T, VW>::load(x + base + a.C, q[1]);
            chan_io<T, VW>::load(x + base + row, q[2]);
            chan_io<T, VW>::load(x + base + row + a.C, q[3]);
            chan_io<T, VW>::load(gy + ((b * a.OH + eh) * a.OW + ew) * a.C + (int64_t)v * VW, g);
#pragma unroll
            for (int e = 0; e < VW; ++e) {
                float m = q[0][e];
                int arg = 0;
#pragma unroll
                for (int k = 1; k < 4; ++k)
                    if (pool_takes(q[k][e], m)) { m = q[k][e]; arg = k; }
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k][e] = (arg == k) ? g[e] : 0.f;
            }
            chan_io<T, VW>::store(gx + base, o[0]);
            chan_io<T, VW>::store(gx + base + a.C, o[1]);
            chan_io<T, VW>::store(gx + base + row, o[2]);
            chan_io<T, VW>::store(gx + base + row + a.C, o[3]);
        } else {
#pragma unroll
            for (int e = 0; e < VW; ++e) o[0][e] = 0.f;
            const bool in_h = 2 * eh + 1 < a.H, in_w = 2 * ew + 1 < a.W;      // (2 eh < H and 2 ew < W by the grid)
            chan_io<T, VW>::store(gx + base, o[0]);
            if (in_w) chan_io<T, VW>::store(gx + base + a.C, o[0]);
            if (in_h) chan_io<T, VW>::store(gx + base + row, o[0]);
            if (in_h && in_w) chan_io<T, VW>::store(gx + base + row + a.C, o[0]);
        }
    }
}

int pool_check(int B, int C, int H, int W, int dtype, bool vec_aligned, PoolArgs* a, int* vw) {
    if (dtype != IDEAS_F32 && dtype != IDEAS_BF16) return IDEAS_E_UNSUPPORTED;
    if (B <= 0 || C <= 0 || H < 2 || W < 2) return IDEAS_E_SHAPE;              // H / 2 and W / 2 must be positive
    *vw = ideas_chan_vw(dtype, C, vec_aligned);
    *a = PoolArgs{B, H, W, C, H / 2, W / 2, C / *vw};
    return IDEAS_OK;
}

unsigned pool_grid(int64_t n) {
    int64_t nblk = ideas_cdiv(n, 256);
    if (nblk > 8192) nblk = 8192;
    return (unsigned)(nblk < 1 ? 1 : nblk);
}

// ---- the head -------------------------------------------------------------------------------------------------------------------
struct LpArgs {
    int64_t P;            // H * W
    int B, C, L, G;       // samples, channels, vectors per pixel, lanes per pixel
    float inv_p;          // 1 / (H W)
};

// the lane's vectors l, l + G, ... of one pixel (zeros past L, and for a pixel past the end)
template <typename T, int VW, int KV>
__device__ __forceinline__ void lp_load(const T* __restrict__ f, int l, int G, int L, bool live, float (&r)[KV][VW]) {
#pragma unroll
    for (int k = 0; k < KV; ++k) {
        const int v = l + k * G;
        if (live && v < L) {
            chan_io<T, VW>::load(f + (int64_t)v * VW, r[k]);
        } else {
#pragma unroll
            for (int e = 0; e < VW; ++e) r[k][e] = 0.f;
        }
    }
}

template <int VW, int KV>
__device__ __forceinline__ void lp_load_w(const float* __restrict__ w, int l, int G, int L, float (&r)[KV][VW]) {
#pragma unroll
    for (int k = 0; k < KV; ++k) {
        const int v = l + k * G;
#pragma unroll
        for (int e = 0; e < VW; ++e) r[k][e] = 0.f;
        if (v < L) {
            if constexpr (VW == 1) {
                r[k][0] = w[v];
            } else {
#pragma unroll
                for (int q = 0; q < VW; q += 4) {
                    const float4 t = *reinterpret_cast<const float4*>(w + (int64_t)v * VW + q);
                    r[k][q] = t.x; r[k][q + 1] = t.y; r[k][q + 2] = t.z; r[k][q + 3] = t.w;
                }
            }
        }
    }
}

template <int VW, int KV>
__device__ __forceinline__ float lp_sqsum(const float (&x)[KV][VW]) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < KV; ++k)
#pragma unroll
        for (int e = 0; e < VW; ++e) s += x[k][e] * x[k][e];
    return s;
}

// pixels in flight per group: as many as the registers of the small per-lane footprints allow
template <int VW, int KV> struct lp_unroll { static constexpr int FWD = (KV * VW <= 8) ? 4 : 1, BWD = (KV * VW <= 8) ? 2 : 1; };

template <typename T, int VW, int KV>
__global__ __launch_bounds__(256) void lpips_fwd_kernel(double* __restrict__ part, const T* __restrict__ f0, const T* __restrict__ f1,
                                                        const float* __restrict__ w, LpArgs a) {
    constexpr int U = lp_unroll<VW, KV>::FWD;
    __shared__ double s_part[4];
    const int l = (int)threadIdx.x & (a.G - 1);
    const int64_t gpb = 256 / a.G;                                     // groups per block
    const int64_t grp = (int64_t)blockIdx.x * gpb + (int)threadIdx.x / a.G;
    const int64_t ngrp = (int64_t)gridDim.x * gpb;
    const int64_t sample = (int64_t)blockIdx.y * a.P * a.C;
    float wv[KV][VW];
    lp_load_w<VW, KV>(w, l, a.G, a.L, wv);
    double acc = 0.0;
    // the trip count is the same for every lane of the block: group_sum() needs all lanes of a wave
    const int64_t ntrips = (a.P + U * ngrp - 1) / (U * ngrp);
    for (int64_t t = 0; t < ntrips; ++t) {
        float x0[U][KV][VW], x1[U][KV][VW];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t pix = grp + (t * U + u) * ngrp;
            const bool live = pix < a.P;
            const int64_t off = sample + (live ? pix : 0) * a.C;
            lp_load<T, VW, KV>(f0 + off, l, a.G, a.L, live, x0[u]);
            lp_load<T, VW, KV>(f1 + off, l, a.G, a.L, live, x1[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float n0 = sqrtf(group_sum(lp_sqsum<VW, KV>(x0[u]), a.G)), n1 = sqrtf(group_sum(lp_sqsum<VW, KV>(x1[u]), a.G));
            const float r0 = 1.f / (n0 + LP_EPS), r1 = 1.f / (n1 + LP_EPS);
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < KV; ++k)
#pragma unroll
                for (int e = 0; e < VW; ++e) {
                    // two rounded products, no FMA contraction: an identical pair gives exactly 0
                    const float dlt = mul_rn(x0[u][k][e], r0) - mul_rn(x1[u][k][e], r1);
                    s += wv[k][e] * (dlt * dlt);
                }
            s = group_sum(s, a.G);
            if (l == 0) acc += (double)s;                  // (zero for a pixel past the end)
        }
    }
    acc = block_sum_256<double, true>(acc, s_part);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

// d[b] = (1/(HW)) * the sum, in index order, of the sample's partials
__global__ __launch_bounds__(256) void lpips_fill_kernel(float* __restrict__ d, const double* __restrict__ part, int B, int nblk, double inv_p) {
    const int b = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (b >= B) return;
    double s = 0.0;
    for (int j = 0; j < nblk; ++j) s += part[(int64_t)b * nblk + j];
    d[b] = (float)(s * inv_p);
}

template <typename T, int VW, int KV>
__global__ __launch_bounds__(256) void lpips_bwd_kernel(T* __restrict__ gf0, T* __restrict__ gf1, const float* __restrict__ gd,
                                                        const T* __restrict__ f0, const T* __restrict__ f1, const float* __restrict__ w,
                                                        LpArgs a) {
    constexpr int U = lp_unroll<VW, KV>::BWD;
    const int l = (int)threadIdx.x & (a.G - 1);
    const int64_t gpb = 256 / a.G;
    const int64_t grp = (int64_t)blockIdx.x * gpb + (int)threadIdx.x / a.G;
    const int64_t ngrp = (int64_t)gridDim.x * gpb;
    const int64_t npix = (int64_t)a.B * a.P;
    float wv[KV][VW];
    lp_load_w<VW, KV>(w, l, a.G, a.L, wv);
    const int64_t ntrips = (npix + U * ngrp - 1) / (U * ngrp);
    for (int64_t t = 0; t < ntrips; ++t) {
        float x0[U][KV][VW], x1[U][KV][VW], sc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t pix = grp + (t * U + u) * ngrp;
            const bool live = pix < npix;
            const int64_t off = (live ? pix : 0) * a.C;
            lp_load<T, VW, KV>(f0 + off, l, a.G, a.L, live, x0[u]);
            lp_load<T, VW, KV>(f1 + off, l, a.G, a.L, live, x1[u]);
            sc[u] = live ? 2.f * gd[pix / a.P] * a.inv_p : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t pix = grp + (t * U + u) * ngrp;
            const float n0 = sqrtf(group_sum(lp_sqsum<VW, KV>(x0[u]), a.G)), n1 = sqrtf(group_sum(lp_sqsum<VW, KV>(x1[u]), a.G));
            const float r0 = 1.f / (n0 + LP_EPS), r1 = 1.f / (n1 + LP_EPS);
            float g[KV][VW], dot0 = 0.f, dot1 = 0.f;
#pragma unroll
            for (int k = 0; k < KV; ++k)
#pragma unroll
                for (int e = 0; e < VW; ++e) {
                    g[k][e] = wv[k][e] * (mul_rn(x0[u][k][e], r0) - mul_rn(x1[u][k][e], r1)) * sc[u];
                    dot0 += g[k][e] * x0[u][k][e];
                    dot1 += g[k][e] * x1[u][k][e];
                }
            dot0 = group_sum(dot0, a.G);
            dot1 = group_sum(dot1, a.G);
            if (pix >= npix) continue;
            // n = 0: the pixel's features are all zero, its gradient is defined as zero
            const float z0 = n0 > 0.f ? r0 : 0.f, c0 = n0 > 0.f ? dot0 * r0 * r0 / n0 : 0.f;
            const float z1 = n1 > 0.f ? r1 : 0.f, c1 = n1 > 0.f ? dot1 * r1 * r1 / n1 : 0.f;
#pragma unroll
            for (int k = 0; k < KV; ++k) {
                const int v = l + k * a.G;
                if (v >= a.L) continue;
                float o[VW];
                if (gf0) {
#pragma unroll
                    for (int e = 0; e < VW; ++e) o[e] = g[k][e] * z0 - x0[u][k][e] * c0;
                    chan_io<T, VW>::store(gf0 + pix * a.C + (int64_t)v * VW, o);
                }
                if (gf1) {
#pragma unroll
                    for (int e = 0; e < VW; ++e) o[e] = x1[u][k][e] * c1 - g[k][e] * z1;
                    chan_io<T, VW>::store(gf1 + pix * a.C + (int64_t)v * VW, o);
                }
            }
        }
    }
}

// shared argument checks; fills the geometry for the vector (vec) or the scalar path; *kv = vectors a lane holds
int lp_check(int B, int C, int H, int W, int dtype, bool vec_aligned, LpArgs* a, int* vw, int* kv) {
    if (dtype != IDEAS_F32 && dtype != IDEAS_BF16) return IDEAS_E_UNSUPPORTED;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || (int64_t)H * W > 0x7fffffffLL || B > 65535) return IDEAS_E_SHAPE;
    if (C > 64 * LP_MAX_LANE_ELEMS) return IDEAS_E_UNSUPPORTED;                 // a pixel of both tensors lives in registers
    *vw = ideas_chan_vw(dtype, C, vec_aligned);
    a->P = (int64_t)H * W;
    a->B = B;
    a->C = C;
    a->L = C / *vw;
    a->G = ideas_lane_group(a->L);
    *kv = (a->L + a->G - 1) / a->G;
    a->inv_p = (float)(1.0 / (double)a->P);
    return IDEAS_OK;
}

// KERNEL<T, VW, KV> with the smallest instantiated KV >= kv; lp_check bounds kv by LP_MAX_LANE_ELEMS / VW (VW = 1: 32, 4: 8, 8: 4)
#define LP_PICK_KV(KERNEL, ...)                                                                                                    \
    do {                                                                                                                           \
        if (kv <= 1) hipLaunchKernelGGL((KERNEL<T, VW, 1>), grid, dim3(256), 0, stream, __VA_ARGS__);                              \
        else if (kv <= 2) hipLaunchKernelGGL((KERNEL<T, VW, 2>), grid, dim3(256), 0, stream, __VA_ARGS__);                         \
        else if (kv <= 4) hipLaunchKernelGGL((KERNEL<T, VW, 4>), grid, dim3(256), 0, stream, __VA_ARGS__);                         \
        else if constexpr (VW <= 4) {                                                                                              \
            if (kv <= 8) hipLaunchKernelGGL((KERNEL<T, VW, 8>), grid, dim3(256), 0, stream, __VA_ARGS__);                          \
            else if constexpr (VW == 1) hipLaunchKernelGGL((KERNEL<T, VW, 32>), grid, dim3(256), 0, stream, __VA_ARGS__);          \
        }                                                                                                                          \
    } while (0)

template <typename T, int VW>
void lp_fwd_launch(int kv, dim3 grid, hipStream_t stream, double* part, const void* f0, const void* f1, const float* w, const LpArgs& a) {
    LP_PICK_KV(lpips_fwd_kernel, part, (const T*)f0, (const T*)f1, w, a);
}

template <typename T, int VW>
void lp_bwd_launch(int kv, dim3 grid, hipStream_t stream, void* gf0, void* gf1, const float* gd, const void* f0, const void* f1,
                   const float* w, const LpArgs& a) {
    LP_PICK_KV(lpips_bwd_kernel, (T*)gf0, (T*)gf1, gd, (const T*)f0, (const T*)f1, w, a);
}
#undef LP_PICK_KV

}  // namespace

extern "C" int ideas_maxpool2x2_fwd(void* y, const void* x, int B, int C, int H, int W, int dtype, void* stream_) {
    PoolArgs a;
    int vw;
    const int rc = pool_check(B, C, H, W, dtype, ideas_aligned16(y) && ideas_aligned16(x), &a, &vw);
    if (rc) return rc;
    if (!y || !x) return IDEAS_E_NULL;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid(pool_grid((int64_t)B * a.OH * a.OW * a.L));
    with_chan(dtype, vw, [&](auto c) {
        using T = typename decltype(c)::type;
        hipLaunchKernelGGL((maxpool_fwd_kernel<T, c.VW>), grid, dim3(256), 0, stream, (T*)y, (const T*)x, a);
    });
    return ideas_launch_status();
}

extern "C" int ideas_maxpool2x2_bwd(void* gx, const void* gy, const void* x, int B, int C, int H, int W, int dtype, void* stream_) {
    PoolArgs a;
    int vw;
    const int rc = pool_check(B, C, H, W, dtype, ideas_aligned16(gx) && ideas_aligned16(gy) && ideas_aligned16(x), &a, &vw);
    if (rc) return rc;
    if (!gx || !gy || !x) return IDEAS_E_NULL;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid(pool_grid((int64_t)B * ((H + 1) / 2) * ((W + 1) / 2) * a.L));
    with_chan(dtype, vw, [&](auto c) {
        using T = typename decltype(c)::type;
        hipLaunchKernelGGL((maxpool_bwd_kernel<T, c.VW>), grid, dim3(256), 0, stream, (T*)gx, (const T*)gy, (const T*)x, a);
    });
    return ideas_launch_status();
}

extern "C" int ideas_lpips_layer_fwd(float* d, void* workspace, const void* f0, const void* f1, const float* w, int B, int C, int H,
                                     int W, int dtype, void* stream_) {
    LpArgs a;
    int vw, kv;
    const int rc = lp_check(B, C, H, W, dtype, ideas_aligned16(f0) && ideas_aligned16(f1) && ideas_aligned16(w), &a, &vw, &kv);
    if (rc) return rc;
    if (!d || !workspace || !f0 || !f1 || !w) return IDEAS_E_NULL;
    hipStream_t stream = (hipStream_t)stream_;
    double* part = (double*)workspace;
    int64_t nblk = ideas_cdiv(a.P, 256 / a.G);
    if (nblk > LP_MAX_BLOCKS) nblk = LP_MAX_BLOCKS;
    const dim3 grid((unsigned)nblk, (unsigned)B);
    with_chan(dtype, vw, [&](auto c) { lp_fwd_launch<typename decltype(c)::type, c.VW>(kv, grid, stream, part, f0, f1, w, a); });
    const int st = ideas_launch_status();
    if (st) return st;
    hipLaunchKernelGGL(lpips_fill_kernel, dim3((unsigned)ideas_cdiv(B, 256)), dim3(256), 0, stream, d, part, B, (int)nblk, 1.0 / (double)a.P);
    return ideas_launch_status();
}

extern "C" int ideas_lpips_layer_bwd(void* gf0, void* gf1, const float* gd, const void* f0, const void* f1, const float* w, int B, int C,
                                     int H, int W, int dtype, void* stream_) {
    LpArgs a;
    int vw, kv;
    const int rc = lp_check(B, C, H, W, dtype,
                            ideas_aligned16(gf0) && ideas_aligned16(gf1) && ideas_aligned16(f0) && ideas_aligned16(f1) && ideas_aligned16(w),
                            &a, &vw, &kv);
    if (rc) return rc;
    if ((!gf0 && !gf1) || !gd || !f0 || !f1 || !w) return IDEAS_E_NULL;
    hipStream_t stream = (hipStream_t)stream_;
    int64_t nblk = ideas_cdiv((int64_t)B * a.P, 256 / a.G);
    if (nblk > 4096) nblk = 4096;
    const dim3 grid((unsigned)nblk);
    with_chan(dtype, vw, [&](auto c) { lp_bwd_launch<typename decltype(c)::type, c.VW>(kv, grid, stream, gf0, gf1, gd, f0, f1, w, a); });
    return ideas_launch_status();
}
