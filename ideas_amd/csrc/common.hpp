// Shared helpers for the gfx950 kernels of libideas_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ideas_hip.h"

#define IDEAS_WAVE 64

static inline int ideas_launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? IDEAS_OK : (int)e;
}

// p on a multiple of N bytes (N a power of two); a null pointer is aligned
template <unsigned N> static inline bool ideas_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & (N - 1u)) == 0; }
static inline bool ideas_aligned16(const void* p) { return ideas_aligned<16>(p); }

static inline int64_t ideas_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Workgroup id -> tile id so that each XCD (block b runs on XCD b % 8, private 4 MiB L2) owns a contiguous band of tiles.
// Bijective for any grid size (the q/rem form of cdna_hip_programming.md T1).
__device__ __forceinline__ int xcd_swizzle(int bid, int nblk) {
    const int q = nblk >> 3, rem = nblk & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    return (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + idx;
}

// Split-K grids of the weight-gradient kernels: every tile of one K split reads the same pixels of gy / x, so the tiles of a
// split should meet in ONE XCD's L2 instead of being dealt round-robin over the eight (each XCD would then fetch the split's
// pixels from HBM itself).  1-D grid of tiles * splits blocks in split-major order, cut into eight contiguous bands by
// xcd_swizzle: XCD k runs splits [k S/8, (k+1) S/8) with all their tiles, dispatched back to back; every XCD gets the same
// number of blocks (+-1) whatever tiles and splits are.  Measured (tools/bench_igemm.py, B = 32): bf16 weight gradient of the
// 128-channel layers at 256x256 384 -> 592 TFLOP/s, 64->128 @256x256 450 -> 647; split-bf16 kernels +2-5 %.
static inline unsigned splitk_grid(int64_t tiles, int64_t splits) { return (unsigned)(tiles * splits); }
__device__ __forceinline__ void splitk_xcd_map(int L, int tiles, int splits, int& tile, int& split) {
    const int l = xcd_swizzle(L, tiles * splits);
    split = l / tiles;
    tile = l - split * tiles;
}

// ---- activation element access for the storage dtypes: f32 arithmetic for f32 / bf16 / f16, f64 for f64 --------------------------------
typedef unsigned short ideas_bf16;                 // one bf16 element in HBM
struct ideas_bf16x4 { uint2 v; };                  // four consecutive bf16 (8 bytes)
__device__ __forceinline__ unsigned ideas_pk_bf16(float a, float b) {          // two f32 -> two RNE bf16 (v_cvt_pk_bf16_f32)
    typedef float f32x2_ __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2_ __attribute__((ext_vector_type(2)));
    const f32x2_ t = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(t, bf16x2_));
}
__device__ __forceinline__ float ideas_bf_lo(unsigned pk) { return __builtin_bit_cast(float, pk << 16); }            // its low element
__device__ __forceinline__ float ideas_bf_hi(unsigned pk) { return __builtin_bit_cast(float, pk & 0xffff0000u); }    // its high element
__device__ __forceinline__ float4 to_f4(float4 v) { return v; }
__device__ __forceinline__ float4 to_f4(ideas_bf16x4 p) {
    return make_float4(__builtin_bit_cast(float, p.v.x << 16), __builtin_bit_cast(float, p.v.x & 0xffff0000u),
                       __builtin_bit_cast(float, p.v.y << 16), __builtin_bit_cast(float, p.v.y & 0xffff0000u));
}
template <typename V> __device__ __forceinline__ V from_f4(float4 v);
template <> __device__ __forceinline__ float4 from_f4<float4>(float4 v) { return v; }
template <> __device__ __forceinline__ ideas_bf16x4 from_f4<ideas_bf16x4>(float4 v) {
    ideas_bf16x4 r;
    r.v = make_uint2(ideas_pk_bf16(v.x, v.y), ideas_pk_bf16(v.z, v.w));
    return r;
}
__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const ideas_bf16* p) { return __builtin_bit_cast(float, (unsigned)(*p) << 16); }
__device__ __forceinline__ float ld1(const _Float16* p) { return (float)*p; }
__device__ __forceinline__ double ld1(const double* p) { return *p; }
__device__ __forceinline__ void st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void st1(ideas_bf16* p, float v) { *p = (ideas_bf16)(ideas_pk_bf16(v, 0.f) & 0xffffu); }
__device__ __forceinline__ void st1(_Float16* p, float v) { *p = (_Float16)v; }                  // one RNE rounding
__device__ __forceinline__ void st1(double* p, double v) { *p = v; }

// eight consecutive 2-byte elements (bf16 or f16) in one 16-byte vector <-> eight f32 (exact widening, RNE narrowing)
__device__ __forceinline__ void unpack8(const uint4& u, float (&f)[8], ideas_bf16) {
    f[0] = __builtin_bit_cast(float, u.x << 16); f[1] = __builtin_bit_cast(float, u.x & 0xffff0000u);
    f[2] = __builtin_bit_cast(float, u.y << 16); f[3] = __builtin_bit_cast(float, u.y & 0xffff0000u);
    f[4] = __builtin_bit_cast(float, u.z << 16); f[5] = __builtin_bit_cast(float, u.z & 0xffff0000u);
    f[6] = __builtin_bit_cast(float, u.w << 16); f[7] = __builtin_bit_cast(float, u.w & 0xffff0000u);
}
__device__ __forceinline__ uint4 pack8(const float (&f)[8], ideas_bf16) {
    return make_uint4(ideas_pk_bf16(f[0], f[1]), ideas_pk_bf16(f[2], f[3]), ideas_pk_bf16(f[4], f[5]), ideas_pk_bf16(f[6], f[7]));
}
typedef _Float16 ideas_f16x8_ __attribute__((ext_vector_type(8)));
typedef float ideas_f32x8_ __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void unpack8(const uint4& u, float (&f)[8], _Float16) {
    const ideas_f32x8_ v = __builtin_convertvector(__builtin_bit_cast(ideas_f16x8_, u), ideas_f32x8_);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = v[e];
}
__device__ __forceinline__ uint4 pack8(const float (&f)[8], _Float16) {
    const ideas_f32x8_ v = {f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7]};
    return __builtin_bit_cast(uint4, __builtin_convertvector(v, ideas_f16x8_));
}
struct ideas_f16x8 { uint4 v; };                   // eight consecutive f16 (16 bytes)

// a 16-byte (f32, f16) or 8-byte (bf16) activation vector as H float4: load / store with one rounding per element
template <typename V> struct vec_io {
    static constexpr int H = 1;
    static __device__ __forceinline__ void load(const V& p, float4 (&o)[1]) { o[0] = to_f4(p); }
    static __device__ __forceinline__ V store(const float4 (&o)[1]) { return from_f4<V>(o[0]); }
};
template <> struct vec_io<ideas_f16x8> {
    static constexpr int H = 2;
    static __device__ __forceinline__ void load(const ideas_f16x8& p, float4 (&o)[2]) {
        float f[8];
        unpack8(p.v, f, _Float16{});
        o[0] = make_float4(f[0], f[1], f[2], f[3]);
        o[1] = make_float4(f[4], f[5], f[6], f[7]);
    }
    static __device__ __forceinline__ ideas_f16x8 store(const float4 (&o)[2]) {
        const float f[8] = {o[0].x, o[0].y, o[0].z, o[0].w, o[1].x, o[1].y, o[1].z, o[1].w};
        return ideas_f16x8{pack8(f, _Float16{})};
    }
};

__device__ __forceinline__ float4 mul4(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
// component-wise select: a ternary on the float4 aggregates becomes a select between two ADDRESSES, which forces
// the staging registers into scratch memory (seen in the ISA as scratch_store + vmcnt(0) after every load)
__device__ __forceinline__ float4 keep4(bool ok, float4 v) {
    return make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
}

constexpr unsigned RSRC_FLAGS = 0x00020000u;   // buffer resource word 3 of the raw buffer accesses: 32-bit data format

// mirror an out-of-range coordinate back into [0,n) (ReflectionPad2d semantics, no edge repeat)
__device__ __forceinline__ int reflect_coord(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return i;
}

// a*b then +c with TWO roundings.  hipcc contracts `a*b + c` into one FMA by default (and __fmul_rn/__fadd_rn are
// plain operators in HIP), which would make a fused conv epilogue differ by 1 ulp from conv -> fused_bias_act.
__device__ __forceinline__ float mul_then_add(float a, float b, float c) {
#pragma clang fp contract(off)
    const float m = a * b;
    return m + c;
}
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// One f32 subtract / multiply / FMA as ONE single-issue VALU instruction that the vectorisers cannot pair.  Written as plain C++, two
// adjacent f32 subtractions (b3.hpp::split2) or multiplies (the modulation scale) are SLP-packed by -O3 into v_pk_add_f32 /
// v_pk_mul_f32, and a packed f32 op issued beside MFMAs costs far more than its two halves (MI355X: two v_pk_add_f32 in an MFMA gap
// +26 cycles against two scalar ones).  Same IEEE operation, same rounding and denormal mode: results are bitwise those of `a - b` /
// `a * b`; the multiply cannot be contracted into an FMA, which keeps mul_rn's guarantee.  Not `volatile`: the compiler may still
// move, merge or drop them.  -DIDEAS_B3_PACKED_F32=1 restores the plain operators (the packed form, for A/B builds).
// RESTRICTION: the compiler's hazard recogniser does not look inside inline assembly (no wait states for MFMA -> VALU read / write of
// the same registers, none for a VALU write that a DPP instruction reads next).  Use them only where they are used now: on staged
// loads and on values computed from them, with results that feed v_cvt_pk_bf16_f32 / LDS stores / plain VALU code -- never on
// MFMA results (an epilogue) and never on a value whose next reader is a DPP instruction (conv_b3_s2fir.hip::hrow1's source).
#ifndef IDEAS_B3_PACKED_F32
#define IDEAS_B3_PACKED_F32 0
#endif
__device__ __forceinline__ float sub1(float a, float b) {
#if IDEAS_B3_PACKED_F32
    return a - b;
#else
    float r;
    asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
#endif
}
__device__ __forceinline__ float mul1(float a, float b) {
#if IDEAS_B3_PACKED_F32
    return mul_rn(a, b);
#else
    float r;
    asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
#endif
}
__device__ __forceinline__ float fma1(float a, float b, float c) {      // fmaf(a, b, c)
#if IDEAS_B3_PACKED_F32
    return fmaf(a, b, c);
#else
    float r;
    asm("v_fma_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
#endif
}

// argument check shared by the convolution entry points (conv_direct.hip)
int check_conv(const ideas_conv_params* p);

// conv_b3.hip: forward-family implicit GEMM with the bf16x3 split contraction (arguments already validated;
// `wplanes` from ideas_b3_split_weights, weight_prep.hip)
int ideas_b3_fwd(void* y, const void* x, const void* wplanes, const float* in_scale, const float* out_scale,
                 const float* bias, const void* resid, const ideas_conv_params* p, hipStream_t stream);
int ideas_b3_fwd_multi(int n, void* y, const void* x, const void* const* wplanes, const float* in_scale, const float* out_scale,
                       const ideas_conv_params* ps, hipStream_t stream);
// conv_b3_pw.hip: 1x1 / stride-1 layers with Cin <= 128 as a flat HBM-bound GEMM (ideas_b3_pw_ok decides; same results as ideas_b3_fwd)
int ideas_b3_pw_ok(const ideas_conv_params* p, const float* in_scale, const float* out_scale, const void* resid);
int ideas_b3_pw_fwd(void* y, const void* x, const void* wplanes, const float* bias, const void* resid, const ideas_conv_params* p,
                    hipStream_t stream);
int ideas_b3_pw_wgrad_ok(const ideas_conv_params* p, const float* in_scale, const float* out_scale);
int ideas_b3_pw_wgrad(float* gw, const void* gy, const void* x, const ideas_conv_params* p, hipStream_t stream);
// conv_b3_s2fir.hip, MODE 1: plain 3x3 / stride-2 / unpadded convs (optionally modulated) on the fused kernel's LDS image, no FIR
int ideas_b3_s2img_ok(const ideas_conv_params* p, const float* in_scale);
int ideas_b3_s2img_fwd(void* y, const void* x, const void* wplanes, const float* in_scale, const float* out_scale, const float* bias,
                       const void* resid, const ideas_conv_params* p, hipStream_t stream);
// conv_b3_tphase.hip: the four phases of a 3x3 / stride-2 / pad-0 transposed conv in one pass over a shared LDS image of the input
// (-1: the launches are not that geometry -> conv_b3_multi_kernel)
int ideas_b3_fwd_tphase(int n, void* y, const void* x, const void* const* wplanes, const float* in_scale, const float* out_scale,
                        const ideas_conv_params* ps, hipStream_t stream, ideas_conv_params* strips, const void** strip_w, int* nstrips);
// conv_b3_wgrad.hip: weight gradient with the split contraction (arguments validated, ideas_b3_wgrad_supported)
int ideas_b3_wgrad(float* gw, const void* gy, const void* x, const float* in_scale, const float* out_scale,
                   const ideas_conv_params* p, hipStream_t stream);
// conv_b3_wgrad3.hip: the same for 3x3 kernels, tap-fused with a rolling window (arguments validated, ideas_b3_wgrad3_supported)
int ideas_b3_wgrad3(float* gw, const void* gy, const void* x, const float* in_scale, const float* out_scale,
                    const ideas_conv_params* p, hipStream_t stream);
// IDEAS_B3_WGRAD3=0 in the environment keeps every weight gradient on conv_b3_wgrad.hip (A/B measurements)
bool ideas_b3_wgrad3_enabled();
// conv_b3_wino.hip: 3x3/s1/p1 Winograd F(2,3) with the split contraction (uplanes from ideas_b3_wino_split_weights)
int ideas_b3_wino_fwd(void* y, const void* x, const void* uplanes, const float* in_scale, const float* out_scale,
                      const float* bias, const void* resid, const ideas_conv_params* p, hipStream_t stream);

// conv_bf16.hip: bf16 mixed-precision family (dtype IDEAS_BF16): bf16 activations, packed bf16 weights (ideas_bf16_pack_weights)
int ideas_bf16_fwd(void* y, const void* x, const void* wpack, int per_image, const float* out_scale, const float* bias,
                   const void* resid, const ideas_conv_params* p, hipStream_t stream);
// conv_bf16_pw.hip: 1x1 / stride-1 layers with 32 / 64 / 128 input channels as a flat HBM-bound GEMM (ideas_bf16_pw_ok decides; same results)
int ideas_bf16_pw_ok(const ideas_conv_params* p, int per_image, const float* out_scale, const void* y, const void* resid);
int ideas_bf16_pw_fwd(void* y, const void* x, const void* wpack, const float* bias, const void* resid, const ideas_conv_params* p,
                      hipStream_t stream);
int ideas_bf16_fwd_multi(int n, void* y, const void* x, const void* const* wpack, int per_image, const float* out_scale,
                         const ideas_conv_params* ps, hipStream_t stream);
int ideas_bf16_wgrad(float* gw, const void* gy, const void* x, const float* in_scale, const float* out_scale,
                     const ideas_conv_params* p, hipStream_t stream);
