// Steganography codec, device side: the message <-> secret-tensor mapping of utils.py:74-97 on PACKED bits, and the container's trip
// through an 8-bit image file (what torchvision's save_image(normalize=True, range=(-1, 1)) writes and ToTensor + Normalize(0.5, 0.5)
// reads back) in one pass.
//
// Packed bits: one row of nbytes = ceil(L * sigma / 8) bytes per image; message bit j of image b is
// (row[b][j >> 3] >> (7 - (j & 7))) & 1, element l owns bits [l * sigma, (l + 1) * sigma), most significant first (the order of
// message[:, i::sigma]); the pad bits of the last byte are written as 0 and never read.
//
// Every arithmetic step is one f32 operation in the reference's order (no contraction), so the results are bitwise those of the host
// functions: see DESIGN.md "Steganography codec".
#include "stream.hpp"
#include "u8.hpp"

namespace {

// sigma (1..8) message bits starting at bit j0 of a packed row: they span at most two bytes
__device__ __forceinline__ unsigned take_bits(const unsigned char* __restrict__ row, int64_t j0, int sigma, int64_t nbytes) {
    const int64_t k = j0 >> 3;
    const int o = (int)(j0 & 7);
    unsigned w = (unsigned)row[k] << 8;
    if (o + sigma > 8 && k + 1 < nbytes) w |= row[k + 1];
    return (w >> (16 - o - sigma)) & ((1u << sigma) - 1u);
}

__global__ __launch_bounds__(256) void bits_to_tensor_kernel(float* __restrict__ z, const unsigned char* __restrict__ bits,
                                                             const float* __restrict__ jitter, int B, int L, int sigma, float step,
                                                             float r, int64_t nbytes) {
    const int64_t n = (int64_t)B * L;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t b = i / L;
        const int64_t l = i - b * L;
        const float num = (float)take_bits(bits + b * nbytes, l * sigma, sigma, nbytes);
        float v;
        {
#pragma clang fp contract(off)
            v = step * (num + 0.5f) - 1.0f;
            if (jitter) {
                const float t = (jitter[i] * r) * 2.0f - r;
                v = v + t;
            }
        }
        z[i] = v;
    }
}

// the reference's decision for one element: clamp, + 1 ROUNDED TO f32, rescale, floor; 2^sigma (z >= 1) belongs to the top bin
__device__ __forceinline__ unsigned decode1(float z, float inv_step, unsigned top) {
    float n;
    {
#pragma clang fp contract(off)
        const float c = fminf(fmaxf(z, -1.0f), 1.0f);      // a NaN comes out as -1: all bits zero, as the reference's >= on a NaN
        n = (c + 1.0f) * inv_step;                         // (c + 1) / step: step is a power of two, the product is that quotient exactly
    }
    const unsigned q = (unsigned)(int)floorf(n);
    return q < top ? q : top;
}

template <typename T>
__global__ __launch_bounds__(256) void tensor_to_bits_kernel(unsigned char* __restrict__ bits, int* __restrict__ n_err,
                                                             const T* __restrict__ z, const unsigned char* __restrict__ ref, int L,
                                                             int sigma, float inv_step, int64_t nbytes) {
    __shared__ int part[4];
    const int b = (int)blockIdx.x;
    const T* zr = z + (int64_t)b * L;
    const int64_t nbit = (int64_t)L * sigma;
    const unsigned top = (1u << sigma) - 1u;
    int cnt = 0;
    for (int64_t k = threadIdx.x; k < nbytes; k += 256) {
        const int64_t j0 = k << 3;
        const int live = (int)(nbit - j0 < 8 ? nbit - j0 : 8);      // message bits of this byte; the rest is padding
        unsigned byte = 0;
        int64_t l = j0 / sigma;
        int i = (int)(j0 - l * sigma);
        unsigned q = decode1(ld1(zr + l), inv_step, top);
        for (int t = 0; t < live; ++t) {
            byte |= ((q >> (sigma - 1 - i)) & 1u) << (7 - t);
            if (++i == sigma && t + 1 < live) {
                i = 0;
                ++l;
                q = decode1(ld1(zr + l), inv_step, top);
            }
        }
        if (bits) bits[(int64_t)b * nbytes + k] = (unsigned char)byte;
        if (n_err) {
            const unsigned mask = (0xff00u >> live) & 0xffu;
            cnt += __popc((byte ^ ref[(int64_t)b * nbytes + k]) & mask);
        }
    }
    if (!n_err) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) n_err[b] = part[0] + part[1] + part[2] + part[3];
}

// one value through the file: the byte that is written (what a reader's ToTensor + Normalize(0.5, 0.5) makes of it: u8.hpp's byte_to_unit)
__device__ __forceinline__ unsigned quant1(float x) {
    float t;
    {
#pragma clang fp contract(off)
        t = fminf(fmaxf(x, -1.0f), 1.0f);                  // a NaN comes out as -1: byte 0
        t = (t + 1.0f) / 2.0f;
        t = t * 255.0f;
        t = t + 0.5f;
        t = fminf(fmaxf(t, 0.0f), 255.0f);
    }
    return (unsigned)(int)t;
}

__device__ __forceinline__ float4 load4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 load4(const ideas_bf16* p) { return to_f4(*reinterpret_cast<const ideas_bf16x4*>(p)); }

// channels-innermost input: the same element order on both sides.  VEC: four elements a lane -- one vector load (16 bytes of f32), one
// 16-byte store of floats and one 4-byte store of bytes, every wave access contiguous -- four such groups a thread so that their loads
// are in flight together, and an element-wise tail; otherwise one element a thread.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void image_to_u8_flat_kernel(unsigned char* __restrict__ u8, float* __restrict__ y,
                                                               const T* __restrict__ x, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t done = 0;
    if (VEC) {
        constexpr int U = 4;
        const int64_t nq = n >> 2;
        auto emit = [&](int64_t q, float4 v) {
            const unsigned b[4] = {quant1(v.x), quant1(v.y), quant1(v.z), quant1(v.w)};
            // (store_bytes' two stores in this kernel's own form, indexed by the quad: through the byte offset the four groups in
            // flight are scheduled otherwise, 16 instructions more -- DESIGN.md 8.8)
            reinterpret_cast<unsigned*>(u8)[q] = pack4(b);
            if (y) reinterpret_cast<float4*>(y)[q] = make_float4(byte_to_unit(b[0]), byte_to_unit(b[1]), byte_to_unit(b[2]), byte_to_unit(b[3]));
        };
        for (int64_t q0 = (int64_t)blockIdx.x * (256 * U) + threadIdx.x; q0 < nq; q0 += stride * U) {
            if (q0 + (U - 1) * 256 < nq) {                 // a whole group: every load is issued before the first use
                float4 v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) v[u] = load4(x + ((q0 + u * 256) << 2));
#pragma unroll
                for (int u = 0; u < U; ++u) emit(q0 + u * 256, v[u]);
            } else {
                for (int64_t q = q0; q < nq; q += 256) emit(q, load4(x + (q << 2)));
            }
        }
        done = nq << 2;
    }
    for (int64_t i = done + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const unsigned q = quant1(ld1(x + i));
        u8[i] = (unsigned char)q;
        if (y) y[i] = byte_to_unit(q);
    }
}

// planar input: one pixel a thread gathers its C planes (each plane's reads are contiguous across the wave)
template <typename T, int C>
__global__ __launch_bounds__(256) void image_to_u8_planar_kernel(unsigned char* __restrict__ u8, float* __restrict__ y,
                                                                 const T* __restrict__ x, int64_t npix, int64_t hw) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += stride) {
        const int64_t b = p / hw;
        const int64_t s = p - b * hw;
        const T* src = x + b * C * hw + s;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const unsigned q = quant1(ld1(src + c * hw));
            u8[p * C + c] = (unsigned char)q;
            if (y) y[p * C + c] = byte_to_unit(q);
        }
    }
}

unsigned flat_grid(int64_t threads) {
    int64_t grid = ideas_cdiv(threads, 256);
    if (grid > 16384) grid = 16384;
    return (unsigned)(grid < 1 ? 1 : grid);
}

template <typename T>
int launch_image(void* u8, float* y, const void* x, int B, int C, int H, int W, int layout, hipStream_t stream) {
    const int64_t hw = (int64_t)H * W, npix = hw * B, n = npix * C;
    unsigned char* o = (unsigned char*)u8;
    const T* in = (const T*)x;
    if (layout == IDEAS_NHWC || C == 1) {                   // (one channel: the two layouts are the same memory)
        if (ideas_aligned16(x) && ideas_aligned16(u8) && ideas_aligned16(y) && n >= 4)
            hipLaunchKernelGGL((image_to_u8_flat_kernel<T, true>), dim3(flat_grid(ideas_cdiv(n >> 2, 4))), dim3(256), 0, stream, o, y, in, n);
        else
            hipLaunchKernelGGL((image_to_u8_flat_kernel<T, false>), dim3(flat_grid(n)), dim3(256), 0, stream, o, y, in, n);
    } else {
        hipLaunchKernelGGL((image_to_u8_planar_kernel<T, 3>), dim3(flat_grid(npix)), dim3(256), 0, stream, o, y, in, npix, hw);
    }
    return ideas_launch_status();
}

}  // namespace

extern "C" int ideas_bits_to_tensor(float* z, const void* bits, const float* jitter, int B, int L, int sigma, float delta,
                                    void* stream_) {
    if (!z || !bits) return IDEAS_E_NULL;
    if (B <= 0 || L <= 0) return IDEAS_E_SHAPE;
    if (sigma < 1 || sigma > 8) return IDEAS_E_UNSUPPORTED;
    const double step = 2.0 / (double)(1 << sigma);
    const float r = (float)(step * (double)delta);           // utils.py: the Python float step * delta meets the f32 tensor rounded once
    const int64_t nbytes = ((int64_t)L * sigma + 7) / 8;
    hipLaunchKernelGGL(bits_to_tensor_kernel, dim3(flat_grid((int64_t)B * L)), dim3(256), 0, (hipStream_t)stream_, z,
                       (const unsigned char*)bits, jitter, B, L, sigma, (float)step, r, nbytes);
    return ideas_launch_status();
}

extern "C" int ideas_tensor_to_bits(void* bits, int* n_err, const void* z, const void* ref_bits, int B, int L, int sigma, int dtype,
                                    void* stream_) {
    if (!z || (!bits && !n_err) || (n_err && !ref_bits)) return IDEAS_E_NULL;
    if (B <= 0 || L <= 0) return IDEAS_E_SHAPE;
    if (sigma < 1 || sigma > 8) return IDEAS_E_UNSUPPORTED;
    if (dtype != IDEAS_F32 && dtype != IDEAS_BF16) return IDEAS_E_UNSUPPORTED;
    const float inv_step = (float)(1 << sigma) / 2.0f;
    const int64_t nbytes = ((int64_t)L * sigma + 7) / 8;
    hipStream_t stream = (hipStream_t)stream_;
    with_dtype(dtype, [&](auto c) {
        using T = typename decltype(c)::type;
        hipLaunchKernelGGL(tensor_to_bits_kernel<T>, dim3((unsigned)B), dim3(256), 0, stream, (unsigned char*)bits, n_err, (const T*)z,
                           (const unsigned char*)ref_bits, L, sigma, inv_step, nbytes);
    });
    return ideas_launch_status();
}

extern "C" int ideas_image_f32_to_u8(void* u8, float* y, const void* x, int B, int C, int H, int W, int layout, int dtype,
                                     void* stream_) {
    if (!u8 || !x) return IDEAS_E_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || (C != 1 && C != 3)) return IDEAS_E_SHAPE;
    if (layout != IDEAS_NCHW && layout != IDEAS_NHWC) return IDEAS_E_UNSUPPORTED;
    if (dtype != IDEAS_F32 && dtype != IDEAS_BF16) return IDEAS_E_UNSUPPORTED;
    return with_dtype(dtype, [&](auto c) { return launch_image<typename decltype(c)::type>(u8, y, x, B, C, H, W, layout, (hipStream_t)stream_); });
}
