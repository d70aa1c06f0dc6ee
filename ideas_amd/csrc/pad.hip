// Adjoint of ReflectionPad2d(p) (models.py:102-106) in NHWC: folds the gradient of the padded tensor
// [B, H+2p, W+2p, C] back onto [B, H, W, C] in one pass.  Row y of the input appears in the padded tensor at
// y+p, and additionally at p-y (for 1 <= y <= p) and at 2(H-1)+p-y (for H-1-p <= y <= H-2); same for columns.
// f32 or bf16 (f32 sums over the up to 3 x 3 sources, rows outer, one rounding at the store); any C and any element alignment.
#include "stream.hpp"

namespace {

// one thread per channel vector of gx (stream.hpp: VW = 4 f32 / 8 bf16 elements, or 1 for any C and any element-aligned pointer)
template <typename T, int VW>
__global__ __launch_bounds__(256) void reflect_fold_kernel(T* __restrict__ gx, const T* __restrict__ gp, int B, int H, int W, int L,
                                                           int pad) {
    const int64_t total = (int64_t)B * H * W * L;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        int64_t r = i;
        const int c = (int)(r % L); r /= L;
        const int x = (int)(r % W); r /= W;
        const int y = (int)(r % H);
        const int b = (int)(r / H);
        int ys[3], xs[3], ny = 0, nx = 0;
        ys[ny++] = y + pad;
        if (y >= 1 && y <= pad) ys[ny++] = pad - y;
        if (y >= H - 1 - pad && y <= H - 2) ys[ny++] = 2 * (H - 1) + pad - y;
        xs[nx++] = x + pad;
        if (x >= 1 && x <= pad) xs[nx++] = pad - x;
        if (x >= W - 1 - pad && x <= W - 2) xs[nx++] = 2 * (W - 1) + pad - x;
        float acc[VW];
#pragma unroll
        for (int e = 0; e < VW; ++e) acc[e] = 0.f;
        for (int a = 0; a < ny; ++a)
            for (int e = 0; e < nx; ++e) {
                float v[VW];
                chan_io<T, VW>::load(gp + ((((int64_t)b * Hp + ys[a]) * Wp + xs[e]) * L + c) * VW, v);
#pragma unroll
                for (int k = 0; k < VW; ++k) acc[k] += v[k];
            }
        chan_io<T, VW>::store(gx + i * VW, acc);
    }
}

}  // namespace

extern "C" int ideas_reflect_fold(void* gx, const void* gpadded, int B, int H, int W, int C, int pad, int dtype,
                                  void* stream) {
    if (dtype != IDEAS_F32 && dtype != IDEAS_BF16) return IDEAS_E_UNSUPPORTED;
    if (!gx || !gpadded) return IDEAS_E_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || pad <= 0 || pad >= H || pad >= W) return IDEAS_E_SHAPE;
    const int vw = ideas_chan_vw(dtype, C, ideas_aligned16(gx) && ideas_aligned16(gpadded));
    const int L = C / vw;
    int64_t grid = ideas_cdiv((int64_t)B * H * W * L, 256);
    if (grid > 16384) grid = 16384;
    with_chan(dtype, vw, [&](auto c) {
        using T = typename decltype(c)::type;
        hipLaunchKernelGGL((reflect_fold_kernel<T, c.VW>), dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, (T*)gx, (const T*)gpadded,
                           B, H, W, L, pad);
    });
    return ideas_launch_status();
}
