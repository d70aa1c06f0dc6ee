// The path endpoints of perceptual path length (stylegan2/ppl.py:71-76 for w-space; its slerp, :16-24, for z-space).  lat [2B][D]
// holds the two ends a, b of path i in rows 2i, 2i + 1; out [2B][D] receives f(a, b, t_i) in row 2i and f(a, b, t_i + eps) in row
// 2i + 1 -- the torch.stack([e0, e1], 1).view(2B, D) order.  The reference issues four strided slices, two lerps of three
// elementwise launches each and a stack (slerp: some thirty launches, ten of them row reductions); here ONE launch, one wave64 per
// path, both outputs from one read of a and b, which stay in registers.  The five row sums of slerp (two norms, the dot, the norm of
// the orthogonal part, the norm of the result: the last once per output) are xor butterflies over the wave: no LDS, no atomics.
//   lerp:  a + (b - a) * t, three roundings in that order (contraction off): bitwise the torch expression.
//   slerp: a, b normalised; d = a . b; p = t acos(d); c = normalize(b - d a); normalize(a cos p + c sin p).  No clamp of d, as in the
//          reference: identical (or opposite) ends give c = 0 / 0 (or acos of more than 1) and a row of NaN there and here --
//          unless their dot product happens to round below 1, which gives a finite row without meaning in both.
#include "stream.hpp"

namespace {

constexpr int LERP = 0, SLERP = 1;

// lane l owns the K chunks of VW elements at (k * 64 + l) * VW: a wave reads 64 consecutive chunks at a time
template <int VW, int K, int MODE>
__global__ __launch_bounds__(256) void path_endpoints_kernel(float* __restrict__ out, const float* __restrict__ lat,
                                                            const float* __restrict__ t, float eps, int B, int D) {
    const int path = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (path >= B) return;                                   // (the whole wave: nothing below meets a barrier)
    const int lane = threadIdx.x & 63;
    const float* pa = lat + (int64_t)2 * path * D;
    const float* pb = pa + D;
    float* o0 = out + (int64_t)2 * path * D;
    float* o1 = o0 + D;
    float a[K][VW], b[K][VW];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = (k * 64 + lane) * VW;
        if (e < D) {                                         // (VW = 4: D % 4 == 0, so the whole chunk is inside the row)
            chan_io<float, VW>::load(pa + e, a[k]);
            chan_io<float, VW>::load(pb + e, b[k]);
        } else {
#pragma unroll
            for (int q = 0; q < VW; ++q) a[k][q] = b[k][q] = 0.f;     // adds nothing to a row sum, never stored
        }
    }
    const float t0 = t[path];
    const float t1 = t0 + eps;                               // the f32 sum of lerp_t[:, None] + args.eps
    if constexpr (MODE == LERP) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int e = (k * 64 + lane) * VW;
            if (e >= D) continue;
            float r0[VW], r1[VW];
#pragma unroll
            for (int q = 0; q < VW; ++q) {
#pragma clang fp contract(off)
                const float d = b[k][q] - a[k][q];
                const float m0 = d * t0, m1 = d * t1;
                r0[q] = a[k][q] + m0;
                r1[q] = a[k][q] + m1;
            }
            chan_io<float, VW>::store(o0 + e, r0);
            chan_io<float, VW>::store(o1 + e, r1);
        }
    } else {
        float sa = 0.f, sb = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int q = 0; q < VW; ++q) { sa += a[k][q] * a[k][q]; sb += b[k][q] * b[k][q]; }
        const float na = sqrtf(wave_sum(sa)), nb = sqrtf(wave_sum(sb));
        float sd = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int q = 0; q < VW; ++q) {
                a[k][q] /= na;
                b[k][q] /= nb;
                sd += a[k][q] * b[k][q];
            }
        const float d = wave_sum(sd);
        const float omega = acosf(d);
        float sc = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int q = 0; q < VW; ++q) {
                b[k][q] -= d * a[k][q];                      // b now holds c, the part of b orthogonal to a
                sc += b[k][q] * b[k][q];
            }
        const float nc = sqrtf(wave_sum(sc));
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int q = 0; q < VW; ++q) b[k][q] /= nc;
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const float p = (side ? t1 : t0) * omega;
            const float cp = cosf(p), sp = sinf(p);
            float sv = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k)
#pragma unroll
                for (int q = 0; q < VW; ++q) {
                    const float v = a[k][q] * cp + b[k][q] * sp;
                    sv += v * v;
                }
            const float nv = sqrtf(wave_sum(sv));
            float* o = side ? o1 : o0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int e = (k * 64 + lane) * VW;
                if (e >= D) continue;
                float r[VW];
#pragma unroll
                for (int q = 0; q < VW; ++q) r[q] = (a[k][q] * cp + b[k][q] * sp) / nv;     // (the same expression as under sv)
                chan_io<float, VW>::store(o + e, r);
            }
        }
    }
}

template <int VW, int K>
void launch(float* out, const float* lat, const float* t, float eps, int B, int D, int mode, hipStream_t s) {
    const dim3 grid((unsigned)ideas_cdiv(B, 4)), block(256);
    auto* kernel = mode == SLERP ? path_endpoints_kernel<VW, K, SLERP> : path_endpoints_kernel<VW, K, LERP>;
    hipLaunchKernelGGL(kernel, grid, block, 0, s, out, lat, t, eps, B, D);
}

// K = the power of two >= chunks a lane: 1 .. 16 (VW = 4) or 1 .. 64 (VW = 1) for D <= IDEAS_PATH_MAX_DIM
template <int VW, int K>
void dispatch(int chunks, float* out, const float* lat, const float* t, float eps, int B, int D, int mode, hipStream_t s) {
    if constexpr (K * VW * 64 < IDEAS_PATH_MAX_DIM) {
        if (chunks > K) return dispatch<VW, 2 * K>(chunks, out, lat, t, eps, B, D, mode, s);
    }
    launch<VW, K>(out, lat, t, eps, B, D, mode, s);
}

}  // namespace

extern "C" int ideas_path_endpoints(float* out, const float* lat, const float* t, float eps, int B, int D, int mode, void* stream_) {
    if (!out || !lat || !t) return IDEAS_E_NULL;
    if (B <= 0 || D <= 0) return IDEAS_E_SHAPE;
    if (D > IDEAS_PATH_MAX_DIM) return IDEAS_E_UNSUPPORTED;
    if (mode != LERP && mode != SLERP) return IDEAS_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream_;
    const int vw = ideas_chan_vw(IDEAS_F32, D, ideas_aligned16(out) && ideas_aligned16(lat));
    const int chunks = (int)ideas_cdiv(D, 64 * vw);
    if (vw == 4) dispatch<4, 1>(chunks, out, lat, t, eps, B, D, mode, s);
    else dispatch<1, 1>(chunks, out, lat, t, eps, B, D, mode, s);
    return ideas_launch_status();
}
