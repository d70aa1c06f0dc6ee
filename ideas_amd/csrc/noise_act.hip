// Noise injection + bias + leaky-ReLU of a StyledConv in one pass, for gfx950 (stylegan2/model.py:280-291 + 335-341: the reference
// runs `out + weight * noise`, the bias add and the activation as separate passes over the feature map).
//
//   forward    out[b,p,c] = lrelu(x[b,p,c] + nw * noise[bn,p] + bias[c], slope) * scale          bn = b ([B,1,H,W]) or 0 ([1,1,H,W])
//   backward   gpre = (out > 0 ? gy : gy * slope) * scale      (sign(out) == sign(pre): the convention of ideas_act_bwd_dot)
//              gx = gpre;  gbias[c] += sum_{b,p} gpre;  gnw = sum_{b,p,c} gpre * noise;  gnoise[bn,p] = nw * sum_c gpre
//
// x / out / gy / gx are channels-innermost [B, P, C] in f32 or bf16, arithmetic is f32; noise, nw (ONE element in device memory,
// never read on the host), bias and every gradient but gx are f32.  HBM-bound: 8 B/elem forward, 12 B/elem backward in f32.
//
// Work split.  A pixel is owned by a GROUP of G = ideas_lane_group(L) lanes, where L = C / VW is the number of channel vectors of
// a pixel (stream.hpp: VW = 4 f32 / 8 bf16 elements, or 1: any C, any alignment); lane l of the group takes the vectors
// l, l + G, ...  G divides 64, so a group never straddles a wave, consecutive groups take consecutive pixels (a
// wave reads contiguous memory), the noise value is loaded once per pixel and lane, and a lane stays on the same channels for the
// whole kernel: the bias lives in registers and the bias gradient is summed in registers -> LDS -> one atomic per channel and
// block, as ideas_fused_bias_act does.  The sum over the channels of a pixel (gnoise) is the xor butterfly inside the group.
//
// gnw is ONE address, so no floating-point atomics: a lane adds (sum of its gpre of a pixel) * noise in double, pixels in index
// order; block_sum_256 combines the block in a fixed order and thread 0 writes one double per block; a
// one-wave kernel adds the <= IDEAS_NOISE_ACT_MAX_PARTIALS partials in a fixed order.  A [1,1,H,W] noise gradient is the sum over b,
// in index order, of the per-sample rows.  out, gx, gnw and gnoise are bitwise reproducible; gbias (float atomics) is not.
#include "stream.hpp"

namespace {

constexpr int NA_U = 4;                                   // pixels in flight per group and trip
constexpr int NA_MAX_BLOCKS = IDEAS_NOISE_ACT_MAX_PARTIALS;

struct NaArgs {
    int64_t npix, P;      // B * H * W, H * W
    int C, L, G;          // channels, vectors per pixel, lanes per pixel
    int noise_per_sample; // 1: noise is [B, P], 0: [1, P]
    float slope, scale;
};

// ---- forward ------------------------------------------------------------------------------------------------------------------
template <typename T, int VW>
__global__ __launch_bounds__(256) void noise_act_fwd_kernel(T* __restrict__ out, const T* __restrict__ x, const float* __restrict__ noise,
                                                            const float* __restrict__ nw_p, const float* __restrict__ bias, NaArgs a) {
    const int l = (int)threadIdx.x & (a.G - 1);
    const int64_t gpb = 256 / a.G;                                     // groups per block
    const int64_t grp = (int64_t)blockIdx.x * gpb + (int)threadIdx.x / a.G;
    const int64_t ngrp = (int64_t)gridDim.x * gpb;
    const float nw = *nw_p;
    for (int64_t pix0 = grp; pix0 < a.npix; pix0 += NA_U * ngrp) {
        float nz[NA_U];
#pragma unroll
        for (int u = 0; u < NA_U; ++u) {
            const int64_t pix = pix0 + u * ngrp;
            nz[u] = 0.f;
            if (pix < a.npix) nz[u] = noise[a.noise_per_sample ? pix : pix % a.P];
        }
        for (int v = l; v < a.L; v += a.G) {
            float bb[VW], xv[NA_U][VW];
            load_f32<VW>(bias + v * VW, bb);
#pragma unroll
            for (int u = 0; u < NA_U; ++u) {
                const int64_t pix = pix0 + u * ngrp;
                if (pix < a.npix) chan_io<T, VW>::load(x + pix * a.C + (int64_t)v * VW, xv[u]);
            }
#pragma unroll
            for (int u = 0; u < NA_U; ++u) {
                const int64_t pix = pix0 + u * ngrp;
                if (pix >= a.npix) break;
                float o[VW];
#pragma unroll
                for (int e = 0; e < VW; ++e) {
                    // x + nw * noise with two roundings (torch's mul, add), + bias, select-multiply, multiply: with nw = 0 the
                    // bits of ideas_fused_bias_act
                    const float t = mul_then_add(nw, nz[u], xv[u][e]) + bb[e];
                    o[e] = mul_rn((t > 0.f) ? t : mul_rn(t, a.slope), a.scale);
                }
                chan_io<T, VW>::store(out + pix * a.C + (int64_t)v * VW, o);
            }
        }
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
// dynamic LDS: 4 doubles (the waves' gnw partials), then C floats (the block's bias gradient)
template <typename T, int VW, bool GNOISE>
__global__ __launch_bounds__(256) void noise_act_bwd_kernel(T* __restrict__ gx, float* __restrict__ gbias, double* __restrict__ part,
                                                            float* __restrict__ gnoise, const T* __restrict__ gy, const T* __restrict__ out,
                                                            const float* __restrict__ noise, const float* __restrict__ nw_p, NaArgs a) {
    extern __shared__ double s_dyn[];
    double* s_part = s_dyn;
    float* s_bg = reinterpret_cast<float*>(s_dyn + 4);
    const int l = (int)threadIdx.x & (a.G - 1);
    const int64_t gpb = 256 / a.G;
    const int64_t grp = (int64_t)blockIdx.x * gpb + (int)threadIdx.x / a.G;
    const int64_t ngrp = (int64_t)gridDim.x * gpb;
    const float nw = GNOISE ? *nw_p : 0.f;
    if (gbias) {
        for (int c = threadIdx.x; c < a.C; c += 256) s_bg[c] = 0.f;
    }
    __syncthreads();
    float accb[VW];                                        // bias gradient of the lane's FIRST vector (all of them when L <= 64)
#pragma unroll
    for (int e = 0; e < VW; ++e) accb[e] = 0.f;
    double accn = 0.0;
    // the trip count is the same for every lane of the block: group_sum() needs all lanes of a wave
    const int64_t ntrips = (a.npix + NA_U * ngrp - 1) / (NA_U * ngrp);
    for (int64_t t = 0; t < ntrips; ++t) {
        const int64_t pix0 = grp + t * NA_U * ngrp;
        float nz[NA_U], csum[NA_U];
#pragma unroll
        for (int u = 0; u < NA_U; ++u) {
            const int64_t pix = pix0 + u * ngrp;
            nz[u] = 0.f;
            csum[u] = 0.f;
            if (pix < a.npix) nz[u] = noise[a.noise_per_sample ? pix : pix % a.P];
        }
        for (int v = l; v < a.L; v += a.G) {
            float g[NA_U][VW], o[NA_U][VW];
#pragma unroll
            for (int u = 0; u < NA_U; ++u) {
                const int64_t pix = pix0 + u * ngrp;
                if (pix < a.npix) {
                    chan_io<T, VW>::load(gy + pix * a.C + (int64_t)v * VW, g[u]);
                    chan_io<T, VW>::load(out + pix * a.C + (int64_t)v * VW, o[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < NA_U; ++u) {
                const int64_t pix = pix0 + u * ngrp;
                if (pix >= a.npix) break;
                float gp[VW], s = 0.f;
#pragma unroll
                for (int e = 0; e < VW; ++e) {
                    gp[e] = mul_rn((o[u][e] > 0.f) ? g[u][e] : mul_rn(g[u][e], a.slope), a.scale);
                    s += gp[e];
                }
                chan_io<T, VW>::store(gx + pix * a.C + (int64_t)v * VW, gp);
                csum[u] += s;
                if (gbias) {
                    if (v == l) {
#pragma unroll
                        for (int e = 0; e < VW; ++e) accb[e] += gp[e];
                    } else {                               // L > 64: the lane's further vectors go to LDS directly
#pragma unroll
                        for (int e = 0; e < VW; ++e) atomicAdd(&s_bg[v * VW + e], gp[e]);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < NA_U; ++u) {
            const int64_t pix = pix0 + u * ngrp;
            accn += (double)csum[u] * (double)nz[u];       // (zero for a pixel past the end)
            if (GNOISE) {
                const float tot = group_sum(csum[u], a.G);
                if (l == 0 && pix < a.npix) gnoise[pix] = mul_rn(nw, tot);
            }
        }
    }
    if (gbias && l < a.L) {
#pragma unroll
        for (int e = 0; e < VW; ++e) atomicAdd(&s_bg[l * VW + e], accb[e]);
    }
    accn = block_sum_256<double, true>(accn, s_part);
    if (threadIdx.x == 0) part[blockIdx.x] = accn;
    if (gbias) {
        for (int c = threadIdx.x; c < a.C; c += 256) {
            const float v = s_bg[c];
            if (v != 0.f) atomicAdd(&gbias[c], v);
        }
    }
}

// gnw = the sum of the blocks' partials: lane j adds its contiguous run in index order, then the xor butterfly (one wave)
__global__ __launch_bounds__(64) void noise_act_fill_kernel(float* __restrict__ gnw, const double* __restrict__ part, int nblk) {
    const int per = (nblk + 63) / 64;
    const int lo = (int)threadIdx.x * per;
    const int hi = lo + per < nblk ? lo + per : nblk;
    double s = 0.0;
    for (int j = lo; j < hi; ++j) s += part[j];
    s = wave_sum(s);
    if (threadIdx.x == 0) *gnw = (float)s;
}

// gnoise[0, p] = sum over b, in index order, of rows[b, p]
__global__ __launch_bounds__(256) void noise_act_batch_sum_kernel(float* __restrict__ gnoise, const float* __restrict__ rows, int B, int64_t P) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += rows[(int64_t)b * P + p];
    gnoise[p] = s;
}

// shared argument checks; fills the geometry for the vector (vec) or the scalar path
int na_check(int B, int C, int H, int W, int noise_batch, int dtype, bool vec_aligned, NaArgs* a, int* vw) {
    if (dtype != IDEAS_F32 && dtype != IDEAS_BF16) return IDEAS_E_UNSUPPORTED;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || (int64_t)H * W > 0x7fffffffLL) return IDEAS_E_SHAPE;
    if (noise_batch != 1 && noise_batch != B) return IDEAS_E_SHAPE;
    if (C > 8192) return IDEAS_E_SHAPE;                                       // the block's bias gradient lives in LDS
    *vw = ideas_chan_vw(dtype, C, vec_aligned);
    a->P = (int64_t)H * W;
    a->npix = (int64_t)B * a->P;
    a->C = C;
    a->L = C / *vw;
    a->G = ideas_lane_group(a->L);
    a->noise_per_sample = noise_batch == B && B > 1;
    return IDEAS_OK;
}

unsigned na_grid(const NaArgs& a, int64_t cap) {
    int64_t nblk = ideas_cdiv(a.npix, (int64_t)(256 / a.G) * NA_U);
    if (nblk > cap) nblk = cap;
    return (unsigned)(nblk < 1 ? 1 : nblk);
}

}  // namespace

extern "C" int ideas_noise_bias_act(void* out, const void* x, const float* noise, const float* noise_weight, const float* bias, int B,
                                    int C, int H, int W, int noise_batch, float slope, float scale, int dtype, void* stream_) {
    NaArgs a;
    int vw;
    const int rc = na_check(B, C, H, W, noise_batch, dtype, ideas_aligned16(x) && ideas_aligned16(out) && ideas_aligned16(bias), &a, &vw);
    if (rc) return rc;
    if (!out || !x || !noise || !noise_weight || !bias) return IDEAS_E_NULL;
    a.slope = slope;
    a.scale = scale;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid(na_grid(a, 4096));
    with_chan(dtype, vw, [&](auto c) {
        using T = typename decltype(c)::type;
        hipLaunchKernelGGL((noise_act_fwd_kernel<T, c.VW>), grid, dim3(256), 0, stream, (T*)out, (const T*)x, noise, noise_weight, bias, a);
    });
    return ideas_launch_status();
}

extern "C" int ideas_noise_bias_act_bwd(void* gx, float* gbias, float* gnw, float* gnoise, void* workspace, const void* gy,
                                        const void* out, const float* noise, const float* noise_weight, int B, int C, int H, int W,
                                        int noise_batch, float slope, float scale, int dtype, void* stream_) {
    NaArgs a;
    int vw;
    const int rc = na_check(B, C, H, W, noise_batch, dtype, ideas_aligned16(gx) && ideas_aligned16(gy) && ideas_aligned16(out), &a, &vw);
    if (rc) return rc;
    if (!gx || !gnw || !workspace || !gy || !out || !noise || !noise_weight) return IDEAS_E_NULL;
    a.slope = slope;
    a.scale = scale;
    hipStream_t stream = (hipStream_t)stream_;
    double* part = (double*)workspace;
    // a [1,1,H,W] noise: the per-sample rows go to the workspace (behind the partials) and are added over b afterwards
    const bool fold = gnoise && !a.noise_per_sample && B > 1;
    float* rows = fold ? reinterpret_cast<float*>(part + NA_MAX_BLOCKS) : gnoise;
    const dim3 grid(na_grid(a, NA_MAX_BLOCKS));
    const size_t lds = 4 * sizeof(double) + (size_t)C * sizeof(float);
    with_chan(dtype, vw, [&](auto c) {
        using T = typename decltype(c)::type;
        auto* kernel = gnoise ? noise_act_bwd_kernel<T, c.VW, true> : noise_act_bwd_kernel<T, c.VW, false>;
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, (T*)gx, gbias, part, rows, (const T*)gy, (const T*)out, noise,
                           noise_weight, a);
    });
    int st = ideas_launch_status();
    if (st) return st;
    hipLaunchKernelGGL(noise_act_fill_kernel, dim3(1), dim3(64), 0, stream, gnw, part, (int)grid.x);
    st = ideas_launch_status();
    if (st || !fold) return st;
    hipLaunchKernelGGL(noise_act_batch_sum_kernel, dim3((unsigned)ideas_cdiv(a.P, 256)), dim3(256), 0, stream, gnoise, rows, B, a.P);
    return ideas_launch_status();
}
