// Minibatch standard deviation of the StyleGAN2 discriminator (stylegan2/model.py:697-705) for gfx950: forward, backward and the
// backward of the backward (R1 differentiates through the block).
//
// x is [B, C, H, W] channels-innermost; sample n = g*M + m belongs to group slot g (outer) and statistic m (inner), G = B / M.
// out is [B, C + feat, H, W] channels-innermost: the first C channels copy x, channel C + f carries s[m, f], the mean over the
// K = (C / feat) * H * W columns of chunk f of the per-column standard deviation over the G samples.
//
// Work split.  A COLUMN is (m, c, h, w): its G values live in registers, so mean, centred values and sd (two-pass: centre first)
// cost no second read; the column arithmetic is double (see column_stats).  The grid is (nblk, M * feat): block (j, m*feat + f) walks the columns q = (h*W + w) * (C/feat) + cc of
// chunk f with stride nblk * 256 -- with the real tail (B = 32, 512 channels, 4x4) that is 32 x 8 blocks, not 8, so the copy of
// the tensor is spread over the chip.  Every reduction over a chunk (s forward, gs backward, t double backward) is a FIXED tree:
// a thread adds its columns in index order, the wave combines with the xor butterfly, thread 0 adds the four waves in order and
// writes one double per block; the small fill kernel adds the <= MBSTD_MAX_BLOCKS partials of a chunk in index order.  No
// floating-point atomics anywhere: two runs give the same bits.
//
// Alignment.  A pixel of `out` / `gout` is C + feat elements: rows are not 16-byte aligned for C = 512 f32 (513 * 4 bytes) nor for
// any bf16 case, so every access here is a scalar element access (a wave still covers 256 contiguous bytes of a pixel row).
#include "stream.hpp"

namespace {

constexpr int MBSTD_MAX_BLOCKS = IDEAS_MBSTD_MAX_PARTIALS;      // partials per (m, f): the fill kernel adds them serially

struct MbArgs {
    int G, M, P, C, feat, nblk;
    float eps;
};

// the G values of one column: loads (sample g at x[base + g * gstride]), mean, centred values u (two-pass) and sd -- in DOUBLE.
// The backward of the backward is a difference of two terms in 1 / sd and u^2 / sd^3 that cancel down to eps / sd^2 of either
// (G = 2: exactly that), so f32 rounding of u = x - mu (6e-8 |x|) would come back multiplied by |x| sd / eps; in double the
// results are good to the rounding of the store.  A column is a few dozen operations and the op is latency-bound: the wider
// arithmetic is not what its time is made of.
template <typename T, int GMAX>
__device__ __forceinline__ void column_stats(const T* __restrict__ x, int64_t base, int64_t gstride, int G, float eps, double (&u)[GMAX],
                                             double& sd) {
    double sum = 0.0;
#pragma unroll
    for (int g = 0; g < GMAX; ++g) {
        u[g] = 0.0;
        if (g < G) { u[g] = (double)ld1(x + base + g * gstride); sum += u[g]; }
    }
    const double inv_g = 1.0 / (double)G;
    const double mu = sum * inv_g;
    double var = 0.0;
#pragma unroll
    for (int g = 0; g < GMAX; ++g) {
        if (g < G) { u[g] -= mu; var += u[g] * u[g]; }
    }
    sd = sqrt(var * inv_g + (double)eps);
}

// ---- forward: copy x into out[:, :C], one partial of sum(sd) per block ------------------------------------------------------
template <typename T, int GMAX>
__global__ __launch_bounds__(256) void mbstd_fwd_kernel(T* __restrict__ out, double* __restrict__ part, const T* __restrict__ x, MbArgs a) {
    __shared__ double s_part[4];
    const int m = blockIdx.y / a.feat, f = blockIdx.y % a.feat;
    const int Cf = a.C / a.feat, Co = a.C + a.feat;
    const int64_t K = (int64_t)a.P * Cf;
    const int64_t gs_x = (int64_t)a.M * a.P * a.C, gs_o = (int64_t)a.M * a.P * Co;
    double acc = 0.0;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < K; q += (int64_t)a.nblk * 256) {
        const int64_t p = q / Cf;
        const int c = f * Cf + (int)(q - p * Cf);
        const int64_t bx = ((int64_t)m * a.P + p) * a.C + c, bo = ((int64_t)m * a.P + p) * Co + c;
        double u[GMAX], sd;
#pragma unroll
        for (int g = 0; g < GMAX; ++g)
            if (g < a.G) st1(out + bo + g * gs_o, ld1(x + bx + g * gs_x));        // exact copy (bf16 -> f32 -> bf16 is the identity)
        column_stats<T, GMAX>(x, bx, gs_x, a.G, a.eps, u, sd);
        acc += sd;
    }
    acc = block_sum_256(acc, s_part);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.y * a.nblk + blockIdx.x] = acc;
}

// ---- fill: out[n, C + f, p] = scale * sum_j part[(n % M) * feat + f][j] -----------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void mbstd_fill_kernel(T* __restrict__ out, const double* __restrict__ part, int64_t n_items, MbArgs a,
                                                         double scale) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_items) return;
    const int f = (int)(i % a.feat);
    const int64_t np = i / a.feat;                    // n * P + p
    const int m = (int)((np / a.P) % a.M);
    const double* src = part + ((int64_t)m * a.feat + f) * a.nblk;
    double s = 0.0;
    for (int j = 0; j < a.nblk; ++j) s += src[j];
    st1(out + np * (a.C + a.feat) + a.C + f, (float)(s * scale));
}

// a[m, f] = (sum over g, p of gout[g*M + m, C + f, p]) / (K * G), the same value in every thread of the block
template <typename T>
__device__ __forceinline__ float extra_channel_mean(const T* __restrict__ gout, int m, int f, const MbArgs& a, double* s_part) {
    const int Co = a.C + a.feat;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < (int64_t)a.G * a.P; i += 256) {
        const int64_t g = i / a.P, p = i - g * a.P;
        acc += (double)ld1(gout + ((g * a.M + m) * a.P + p) * Co + a.C + f);
    }
    acc = block_sum_256(acc, s_part);
    const double KG = (double)a.P * (a.C / a.feat) * a.G;
    return (float)(acc / KG);
}

// ---- backward: gx = gout[:, :C] + a * u / sd; block column 0 stores a[m, f] for the double backward -------------------------
template <typename T, int GMAX>
__global__ __launch_bounds__(256) void mbstd_bwd_kernel(T* __restrict__ gx, float* __restrict__ a_out, const T* __restrict__ gout,
                                                        const T* __restrict__ x, MbArgs a) {
    __shared__ double s_part[4];
    const int m = blockIdx.y / a.feat, f = blockIdx.y % a.feat;
    const int Cf = a.C / a.feat, Co = a.C + a.feat;
    const int64_t K = (int64_t)a.P * Cf;
    const int64_t gs_x = (int64_t)a.M * a.P * a.C, gs_o = (int64_t)a.M * a.P * Co;
    const float am = extra_channel_mean(gout, m, f, a, s_part);
    if (blockIdx.x == 0 && threadIdx.x == 0) a_out[blockIdx.y] = am;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < K; q += (int64_t)a.nblk * 256) {
        const int64_t p = q / Cf;
        const int c = f * Cf + (int)(q - p * Cf);
        const int64_t bx = ((int64_t)m * a.P + p) * a.C + c, bo = ((int64_t)m * a.P + p) * Co + c;
        double u[GMAX], sd;
        column_stats<T, GMAX>(x, bx, gs_x, a.G, a.eps, u, sd);
        const double r = (double)am / sd;
#pragma unroll
        for (int g = 0; g < GMAX; ++g)
            if (g < a.G) st1(gx + bx + g * gs_x, (float)((double)ld1(gout + bo + g * gs_o) + r * u[g]));
    }
}

// ---- backward of the backward, v = ggx:
//   dgout[:, :C] = v;  partial of sum_g v u / sd per block (-> t through the fill kernel);
//   dx = a * ((v - mean_g v) / sd - u * (sum_g v u) / (G sd^3))
template <typename T, int GMAX>
__global__ __launch_bounds__(256) void mbstd_bwd2_kernel(T* __restrict__ dgout, T* __restrict__ dx, double* __restrict__ part,
                                                         const T* __restrict__ v, const T* __restrict__ x, const float* __restrict__ a_in,
                                                         MbArgs a) {
    __shared__ double s_part[4];
    const int m = blockIdx.y / a.feat, f = blockIdx.y % a.feat;
    const int Cf = a.C / a.feat, Co = a.C + a.feat;
    const int64_t K = (int64_t)a.P * Cf;
    const int64_t gs_x = (int64_t)a.M * a.P * a.C, gs_o = (int64_t)a.M * a.P * Co;
    const float am = a_in[blockIdx.y];
    const double inv_g = 1.0 / (double)a.G;
    double acc = 0.0;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < K; q += (int64_t)a.nblk * 256) {
        const int64_t p = q / Cf;
        const int c = f * Cf + (int)(q - p * Cf);
        const int64_t bx = ((int64_t)m * a.P + p) * a.C + c, bo = ((int64_t)m * a.P + p) * Co + c;
        double u[GMAX], vv[GMAX], sd;
        column_stats<T, GMAX>(x, bx, gs_x, a.G, a.eps, u, sd);
        double vsum = 0.0, dot = 0.0;
#pragma unroll
        for (int g = 0; g < GMAX; ++g) {
            vv[g] = 0.0;
            if (g < a.G) {
                const float raw = ld1(v + bx + g * gs_x);
                st1(dgout + bo + g * gs_o, raw);
                vv[g] = (double)raw;
                vsum += vv[g];
                dot += vv[g] * u[g];
            }
        }
        const double inv_sd = 1.0 / sd;
        const double vbar = vsum * inv_g;
        const double w = dot * inv_g * inv_sd * inv_sd * inv_sd;
        acc += dot * inv_sd;
#pragma unroll
        for (int g = 0; g < GMAX; ++g)
            if (g < a.G) st1(dx + bx + g * gs_x, (float)((double)am * ((vv[g] - vbar) * inv_sd - u[g] * w)));
    }
    acc = block_sum_256(acc, s_part);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.y * a.nblk + blockIdx.x] = acc;
}

// shared argument checks; fills the launch geometry
int mb_check(int B, int C, int H, int W, int group, int feat, int dtype, MbArgs* a) {
    if (dtype != IDEAS_F32 && dtype != IDEAS_BF16) return IDEAS_E_UNSUPPORTED;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || group <= 0 || feat <= 0) return IDEAS_E_SHAPE;
    const int G = B < group ? B : group;
    if (B % G != 0 || C % feat != 0) return IDEAS_E_SHAPE;
    if (G > 16) return IDEAS_E_UNSUPPORTED;                                   // the group is held in registers
    const int M = B / G;
    if ((int64_t)M * feat > 65535 || (int64_t)H * W > 0x7fffffffLL) return IDEAS_E_SHAPE;
    const int64_t K = (int64_t)(C / feat) * H * W;
    int64_t nblk = ideas_cdiv(K, 256);
    if (nblk > MBSTD_MAX_BLOCKS) nblk = MBSTD_MAX_BLOCKS;
    *a = MbArgs{G, M, H * W, C, feat, (int)nblk, 0.f};
    return IDEAS_OK;
}

template <typename T>
int mb_fill(void* out, const double* part, int B, const MbArgs& a, double scale, hipStream_t stream) {
    const int64_t n_items = (int64_t)B * a.P * a.feat;
    const int64_t grid = ideas_cdiv(n_items, 256);
    if (grid > 0x7fffffffLL) return IDEAS_E_SHAPE;
    hipLaunchKernelGGL(mbstd_fill_kernel<T>, dim3((unsigned)grid), dim3(256), 0, stream, (T*)out, part, n_items, a, scale);
    return ideas_launch_status();
}

}  // namespace

// KERNEL<T, 4> for G <= 4 (the discriminator's group), KERNEL<T, 16> above
#define MB_LAUNCH(KERNEL, T, ...)                                                                                                  \
    do {                                                                                                                           \
        const dim3 grid((unsigned)a.nblk, (unsigned)(a.M * a.feat));                                                               \
        if (a.G <= 4) hipLaunchKernelGGL((KERNEL<T, 4>), grid, dim3(256), 0, stream, __VA_ARGS__);                                 \
        else hipLaunchKernelGGL((KERNEL<T, 16>), grid, dim3(256), 0, stream, __VA_ARGS__);                                         \
    } while (0)

namespace {

template <typename T>
int mb_fwd(void* out, double* part, const void* x, int B, const MbArgs& a, hipStream_t stream) {
    MB_LAUNCH(mbstd_fwd_kernel, T, (T*)out, part, (const T*)x, a);
    const int rc = ideas_launch_status();
    if (rc) return rc;
    return mb_fill<T>(out, part, B, a, 1.0 / ((double)a.P * (a.C / a.feat)), stream);
}

template <typename T>
int mb_bwd(void* gx, float* a_out, const void* gout, const void* x, const MbArgs& a, hipStream_t stream) {
    MB_LAUNCH(mbstd_bwd_kernel, T, (T*)gx, a_out, (const T*)gout, (const T*)x, a);
    return ideas_launch_status();
}

template <typename T>
int mb_bwd2(void* dgout, void* dx, double* part, const void* ggx, const void* x, const float* a_in, int B, const MbArgs& a,
            hipStream_t stream) {
    MB_LAUNCH(mbstd_bwd2_kernel, T, (T*)dgout, (T*)dx, part, (const T*)ggx, (const T*)x, a_in, a);
    const int rc = ideas_launch_status();
    if (rc) return rc;
    return mb_fill<T>(dgout, part, B, a, 1.0 / ((double)a.P * (a.C / a.feat) * a.G), stream);
}

}  // namespace
#undef MB_LAUNCH

extern "C" int ideas_mbstd_fwd(void* out, void* workspace, const void* x, int B, int C, int H, int W, int group, int feat, float eps,
                               int dtype, void* stream_) {
    MbArgs a;
    const int rc = mb_check(B, C, H, W, group, feat, dtype, &a);
    if (rc) return rc;
    if (!out || !workspace || !x) return IDEAS_E_NULL;
    a.eps = eps;
    return with_dtype(dtype, [&](auto c) { return mb_fwd<typename decltype(c)::type>(out, (double*)workspace, x, B, a, (hipStream_t)stream_); });
}

extern "C" int ideas_mbstd_bwd(void* gx, float* a_out, const void* gout, const void* x, int B, int C, int H, int W, int group, int feat,
                               float eps, int dtype, void* stream_) {
    MbArgs a;
    const int rc = mb_check(B, C, H, W, group, feat, dtype, &a);
    if (rc) return rc;
    if (!gx || !a_out || !gout || !x) return IDEAS_E_NULL;
    a.eps = eps;
    return with_dtype(dtype, [&](auto c) { return mb_bwd<typename decltype(c)::type>(gx, a_out, gout, x, a, (hipStream_t)stream_); });
}

extern "C" int ideas_mbstd_bwd2(void* dgout, void* dx, void* workspace, const void* ggx, const void* x, const float* a_in, int B, int C,
                                int H, int W, int group, int feat, float eps, int dtype, void* stream_) {
    MbArgs a;
    const int rc = mb_check(B, C, H, W, group, feat, dtype, &a);
    if (rc) return rc;
    if (!dgout || !dx || !workspace || !ggx || !x || !a_in) return IDEAS_E_NULL;
    a.eps = eps;
    return with_dtype(dtype, [&](auto c) {
        return mb_bwd2<typename decltype(c)::type>(dgout, dx, (double*)workspace, ggx, x, a_in, B, a, (hipStream_t)stream_);
    });
}
