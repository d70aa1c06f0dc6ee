// Channel attacks on the 8-bit container, device side: a baseline-JPEG (4:4:4) encode-decode round trip in one launch, and the
// per-pixel attacks (intensity, additive Gaussian noise, salt and pepper) in one streaming launch.  The model of the round trip is
// stated step by step in include/ideas_hip.h ("Channel attacks") and restated in numpy by tests/attacks_ref.py.
//
// The round trip's lane mapping, tables, colour conversion, row I/O, tile walk and the block's way through LDS are jpeg_block.hpp's,
// shared with attack_jpeg.hip; this file holds the f32 model's arithmetic (f32_arith), the kernel's planes and the launchers.  The
// container's byte stores are u8.hpp's.  DESIGN.md "Channel attacks".
#include "jpeg_block.hpp"

namespace {

// cos(n pi / 16).  The 8-point transforms below are UNNORMALISED: t_k = sum_j b_k(j) x_j with b_0 = 1, b_4 = (+ - - + + - - +) and
// b_k(j) = cos((2 j + 1) k pi / 16) otherwise; the orthonormal DCT is alpha_k t_k with alpha_0 = alpha_4 = 1 / (2 sqrt 2) and
// alpha_k = 1 / 2.  So the rows 0 and 4 of integer samples are integers, and the product alpha_u alpha_v of the four coefficients with
// u, v in {0, 4} is exactly 1 / 8 instead of the f32 square of 0.35355338.
constexpr float C1 = 0.98078528040323043f, C2 = 0.92387953251128674f, C3 = 0.83146961230254524f, C5 = 0.55557023301960218f,
                C6 = 0.38268343236508978f, C7 = 0.19509032201612825f;
constexpr float SCALE_ONE = 0.17677669529663687f;           // alpha_u alpha_v with exactly one index in {0, 4}: 1 / (4 sqrt 2)
constexpr float SCALE_NONE = 0.25f;                          // ... with none

__device__ __forceinline__ void fdct8(const float (&x)[8], float (&t)[8]) {
    const float s0 = x[0] + x[7], s1 = x[1] + x[6], s2 = x[2] + x[5], s3 = x[3] + x[4];
    const float d0 = x[0] - x[7], d1 = x[1] - x[6], d2 = x[2] - x[5], d3 = x[3] - x[4];
    const float e0 = s0 + s3, e1 = s1 + s2, e2 = s0 - s3, e3 = s1 - s2;
    t[0] = e0 + e1;
    t[4] = e0 - e1;
    t[2] = C2 * e2 + C6 * e3;
    t[6] = C6 * e2 - C2 * e3;
    t[1] = C1 * d0 + C3 * d1 + C5 * d2 + C7 * d3;
    t[3] = C3 * d0 - C7 * d1 - C1 * d2 - C5 * d3;
    t[5] = C5 * d0 - C1 * d1 + C7 * d2 + C3 * d3;
    t[7] = C7 * d0 - C5 * d1 + C3 * d2 - C1 * d3;
}

// x_j = sum_k b_k(j) e_k: with e_1, e_2, e_3, e_5, e_6, e_7 zero every step is an addition of the two others, exact on eighths
__device__ __forceinline__ void idct8(const float (&e)[8], float (&x)[8]) {
    const float a0 = e[0] + e[4], a1 = e[0] - e[4];
    const float b0 = C2 * e[2] + C6 * e[6], b1 = C6 * e[2] - C2 * e[6];
    const float ev0 = a0 + b0, ev1 = a1 + b1, ev2 = a1 - b1, ev3 = a0 - b0;
    const float o0 = C1 * e[1] + C3 * e[3] + C5 * e[5] + C7 * e[7];
    const float o1 = C3 * e[1] - C7 * e[3] - C1 * e[5] - C5 * e[7];
    const float o2 = C5 * e[1] - C1 * e[3] + C7 * e[5] + C3 * e[7];
    const float o3 = C7 * e[1] - C5 * e[3] + C3 * e[5] - C1 * e[7];
    x[0] = ev0 + o0; x[7] = ev0 - o0;
    x[1] = ev1 + o1; x[6] = ev1 - o1;
    x[2] = ev2 + o2; x[5] = ev2 - o2;
    x[3] = ev3 + o3; x[4] = ev3 - o3;
}

// The f32 model as block_roundtrip's arithmetic.  tq: the plane's table; rc: this lane's r as a COLUMN index is 0 or 4
struct f32_arith {
    using T = float;
    const float* tq;
    bool rc;
    __device__ __forceinline__ void rows_fwd(const int (&v)[8], float (&g)[8]) const {
        float a[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = (float)(v[j] - 128);
        fdct8(a, g);
    }
    // a[u] becomes the unnormalised T(u, r)
    __device__ __forceinline__ void cols_fwd(const float (&g)[8], float (&a)[8]) const { fdct8(g, a); }
    __device__ __forceinline__ void quant_dequant(float (&a)[8], short (&qs)[8], int r) const {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float T = tq[u * 8 + r];
            const bool ru = u == 0 || u == 4;
            const float scale = ru ? SCALE_ONE : (rc ? SCALE_ONE : SCALE_NONE);
            const float F = a[u] * scale;
            float q = copysignf(floorf(fabsf(F) / T + 0.5f), F);
            float e = (q * T) * scale;
            if (ru && rc) {                                  // F = S / 8, S an integer: quantised in integers, dequantised in eighths
                const int S = (int)a[u], iT = (int)T;
                const int m = ((S < 0 ? -S : S) + 4 * iT) / (8 * iT);
                const int qi = S < 0 ? -m : m;
                q = (float)qi;
                e = (float)(qi * iT) * 0.125f;
            }
            qs[u] = (short)(int)q;
            a[u] = e;
        }
    }
    __device__ __forceinline__ void cols_inv(const float (&a)[8], float (&g)[8]) const { idct8(a, g); }
    __device__ __forceinline__ void rows_inv(const float (&a)[8], int (&v)[8]) const {
        float g[8];
        idct8(a, g);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float w = floorf((g[j] + 128.0f) + 0.5f);
            v[j] = (int)fminf(fmaxf(w, 0.0f), 255.0f);
        }
    }
};

// VEC: W % 8 == 0, x and out 8-byte aligned, y 16-byte aligned: a lane's 8 pixels are C 8-byte words and 2 C float4
template <int C, bool VEC>
__global__ __launch_bounds__(256) void jpeg_roundtrip_kernel(unsigned char* __restrict__ out, float* __restrict__ y,
                                                             short* __restrict__ coef, const unsigned char* __restrict__ x, int H, int W,
                                                             int qscale, int64_t ntiles) {
    __shared__ __attribute__((aligned(16))) float s_tile[2][4][8 * TILE_LD];      // [forward | inverse][wave][block][8][8]
    __shared__ float s_q[2][64];
    __shared__ float s_unit[256];                            // byte -> received f32, not 8 C times a lane
    fill_unit(s_unit);
    if (threadIdx.x < 128) s_q[threadIdx.x >> 6][threadIdx.x & 63] = (float)jpeg_table_entry(threadIdx.x, qscale);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, blk = lane & 7, r = lane >> 3;
    float* fw = &s_tile[0][wave][blk * TILE_LD];
    float* iv = &s_tile[1][wave][blk * TILE_LD];
    const int bwn = (W + 7) >> 3, bhn = (H + 7) >> 3, txn = (bwn + 7) >> 3;

    for (int64_t t0 = tile_first(); t0 < ntiles; t0 += tile_step()) {
        const jpeg_tile t(t0, wave, lane, ntiles, txn, bhn, bwn);
        const int64_t row_in = (t.b * H + (t.yy < H ? t.yy : H - 1)) * W;        // replicated last row

        int pl[C][8];                                        // the planes: Y (Cb Cr), 0..255
        {
            int px[C][8];
            load8<C, VEC>(x + row_in * C, t.x0, W, px);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if constexpr (C == 3) {
                    pl[0][j] = luma_of(px[0][j], px[1][j], px[2][j]);
                    pl[1][j] = cb_of(px[0][j], px[1][j], px[2][j]);
                    pl[2][j] = cr_of(px[0][j], px[1][j], px[2][j]);
                } else {
                    pl[0][j] = px[0][j];
                }
            }
        }
#pragma unroll
        for (int p = 0; p < C; ++p) {
            block_roundtrip(pl[p], f32_arith{s_q[p > 0], (r & 3) == 0}, fw, iv, r, coef && t.live,
                            coef + ((((t.b * C + p) * bhn + t.by) * bwn + t.bx) * 64 + r));
        }
        unsigned ob[8 * C];                                  // the bytes of this lane's row, pixel-major
        ycc_to_rgb<C>(pl, ob);
        if (t.live && t.yy < H) store8<C, VEC>(out, y, ((t.b * H + t.yy) * W + t.x0) * C, ob, t.x0, W, s_unit);
    }
}

template <int C>
int launch_jpeg(void* out, float* y, short* coef, const void* x, int B, int H, int W, int quality, hipStream_t stream) {
    const int qscale = jpeg_qscale(quality);
    const int64_t bwn = (W + 7) / 8, bhn = (H + 7) / 8;
    const int64_t ntiles = (int64_t)B * bhn * ideas_cdiv(bwn, 8);
    int64_t grid = ideas_cdiv(ntiles, 4);
    if (grid > 16384) grid = 16384;
    const bool vec = W % 8 == 0 && ideas_aligned<8>(x) && ideas_aligned<8>(out) && ideas_aligned16(y);
    if (vec)
        hipLaunchKernelGGL((jpeg_roundtrip_kernel<C, true>), dim3((unsigned)grid), dim3(256), 0, stream, (unsigned char*)out, y, coef,
                           (const unsigned char*)x, H, W, qscale, ntiles);
    else
        hipLaunchKernelGGL((jpeg_roundtrip_kernel<C, false>), dim3((unsigned)grid), dim3(256), 0, stream, (unsigned char*)out, y, coef,
                           (const unsigned char*)x, H, W, qscale, ntiles);
    return ideas_launch_status();
}

// ---- pixel attacks ---------------------------------------------------------------------------------------------------------------
// one byte through intensity and noise: every step one f32 operation, in the order of the header
__device__ __forceinline__ unsigned attack1(unsigned x, float gain, float offset, float sigma, bool noisy, float nz) {
    float t;
    {
#pragma clang fp contract(off)
        t = ((float)x - 127.5f) * gain;
        t = t + 127.5f;
        t = t + offset;
        if (noisy) {
            const float s = sigma * nz;
            t = t + s;
        }
        t = t + 0.5f;
        t = fminf(fmaxf(t, 0.0f), 255.0f);                   // a NaN comes out as 0
    }
    return (unsigned)(int)t;
}

// salt and pepper: one draw decides all channels of a pixel
__device__ __forceinline__ unsigned salt_pepper(unsigned v, float uu, float lo, float hi) { return uu < lo ? 0u : (uu >= hi ? 255u : v); }

// VEC: four pixels a lane -- C 4-byte words of bytes, C float4 of noise, one float4 of draws, C float4 of y -- and a pixel-wise tail;
// otherwise one pixel a thread
template <int C, bool VEC>
__global__ __launch_bounds__(256) void pixel_attack_kernel(unsigned char* __restrict__ out, float* __restrict__ y,
                                                           const unsigned char* __restrict__ x, const float* __restrict__ noise,
                                                           const float* __restrict__ u, int64_t npix, float gain, float offset,
                                                           float sigma, float sp) {
    const float lo = sp / 2.0f, hi = 1.0f - lo;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t done = 0;
    if constexpr (VEC) {
        const int64_t nq = npix >> 2;
        for (int64_t q = tid; q < nq; q += stride) {
            unsigned w[C];
            float nz[4 * C], uu[4];
#pragma unroll
            for (int k = 0; k < C; ++k) w[k] = reinterpret_cast<const unsigned*>(x)[q * C + k];
            if (noise) {
#pragma unroll
                for (int k = 0; k < C; ++k) {
                    const float4 v = reinterpret_cast<const float4*>(noise)[q * C + k];
                    nz[4 * k] = v.x; nz[4 * k + 1] = v.y; nz[4 * k + 2] = v.z; nz[4 * k + 3] = v.w;
                }
            }
            if (u) {
                const float4 v = reinterpret_cast<const float4*>(u)[q];
                uu[0] = v.x; uu[1] = v.y; uu[2] = v.z; uu[3] = v.w;
            }
            unsigned ob[4 * C];
#pragma unroll
            for (int e = 0; e < 4 * C; ++e) {
                ob[e] = attack1(byte_of(w, e), gain, offset, sigma, noise != nullptr, noise ? nz[e] : 0.0f);
                if (u) ob[e] = salt_pepper(ob[e], uu[e / C], lo, hi);
            }
#pragma unroll
            for (int k = 0; k < C; ++k) store_bytes<4, 4>(out, y, (q * C + k) * 4, ob + 4 * k, 4, unit_direct{});     // word by word
        }
        done = nq << 2;
    }
    for (int64_t p = done + tid; p < npix; p += stride) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int64_t i = p * C + c;
            unsigned v = attack1(x[i], gain, offset, sigma, noise != nullptr, noise ? noise[i] : 0.0f);
            if (u) v = salt_pepper(v, u[p], lo, hi);
            out[i] = (unsigned char)v;
            if (y) y[i] = byte_to_unit(v);
        }
    }
}

template <int C>
int launch_pixel(void* out, float* y, const void* x, const float* noise, const float* u, int64_t npix, float gain, float offset,
                 float sigma, float sp, hipStream_t stream) {
    const bool vec = npix >= 4 && ideas_aligned<4>(x) && ideas_aligned<4>(out) && ideas_aligned16(y) && ideas_aligned16(noise) && ideas_aligned16(u);
    int64_t grid = ideas_cdiv(vec ? npix >> 2 : npix, 256);
    if (grid > 16384) grid = 16384;
    if (vec)
        hipLaunchKernelGGL((pixel_attack_kernel<C, true>), dim3((unsigned)grid), dim3(256), 0, stream, (unsigned char*)out, y,
                           (const unsigned char*)x, noise, u, npix, gain, offset, sigma, sp);
    else
        hipLaunchKernelGGL((pixel_attack_kernel<C, false>), dim3((unsigned)grid), dim3(256), 0, stream, (unsigned char*)out, y,
                           (const unsigned char*)x, noise, u, npix, gain, offset, sigma, sp);
    return ideas_launch_status();
}

}  // namespace

extern "C" int ideas_jpeg_roundtrip(void* out_u8, float* y, short* coef, const void* x_u8, int B, int C, int H, int W, int quality,
                                    void* stream_) {
    if (!x_u8 || !out_u8) return IDEAS_E_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || (C != 1 && C != 3)) return IDEAS_E_SHAPE;
    if (quality < 1 || quality > 100) return IDEAS_E_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    return C == 3 ? launch_jpeg<3>(out_u8, y, coef, x_u8, B, H, W, quality, stream)
                  : launch_jpeg<1>(out_u8, y, coef, x_u8, B, H, W, quality, stream);
}

extern "C" int ideas_pixel_attack(void* out_u8, float* y, const void* x_u8, const float* noise, const float* u, int B, int C, int H,
                                  int W, float gain, float offset, float sigma, float sp, void* stream_) {
    if (!x_u8 || !out_u8) return IDEAS_E_NULL;
    if ((!noise && sigma != 0.0f) || (!u && sp != 0.0f)) return IDEAS_E_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || (C != 1 && C != 3)) return IDEAS_E_SHAPE;
    const int64_t npix = (int64_t)B * H * W;
    hipStream_t stream = (hipStream_t)stream_;
    return C == 3 ? launch_pixel<3>(out_u8, y, x_u8, noise, u, npix, gain, offset, sigma, sp, stream)
                  : launch_pixel<1>(out_u8, y, x_u8, noise, u, npix, gain, offset, sigma, sp, stream);
}
