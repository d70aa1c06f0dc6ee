// Shared pieces of the split-bf16 ("b3") kernels: exact 3-way f32 -> bf16 split, buffer loads, plane-pair order.
#pragma once
#include "common.hpp"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int BK = 16;     // f32 K depth of one pipeline step = K of one bf16 MFMA
constexpr int ROWB = 32;   // bytes per LDS row (16 bf16)

// The staging arithmetic that runs beside MFMAs (the residuals of the split, the modulation scale, the FIR sum of conv_b3_s2fir.hip) as single-issue instructions
// (common.hpp::sub1 / mul1 / fma1).  A translation unit whose kernels measured no gain from it defines B3_UNPACK_F32 0 before including
// this header and keeps the plain operators, which -O3 packs in pairs.  Census of the training step, default against the packed build
// (-DIDEAS_B3_PACKED_F32=1) of the same tree, profiles/unpack_f32_family_ab.txt section 3: the tap-fused weight gradient -1.5 %
// (stride 1) / -9.8 % (stride 2), the fused Blur + stride-2 kernel -9.0 % (all of it from its producers' FIR sum; -3 % on the MODE 1
// launches, which have no FIR).  A probe that un-packed one file at a time with -fno-slp-vectorize (section 1) showed nothing beyond
// the spread of two runs of the same library for the generic, flat 1x1, generic weight-gradient and Winograd kernels: they keep the
// plain operators.  The transposed-phase kernel gained 0.4 % in the probe and nothing in the committed form; its helpers are on
// for another reason (see conv_b3_tphase.hip).
// (These inline functions differ between translation units with B3_UNPACK_F32.  That is sound only because every one is
// __forceinline__ device code in an anonymous namespace and the library is built WITHOUT relocatable device code (-fgpu-rdc): no
// definition is ever shared across files.)
#ifndef B3_UNPACK_F32
#define B3_UNPACK_F32 1
#endif
__device__ __forceinline__ float b3_sub(float a, float b) { return B3_UNPACK_F32 ? sub1(a, b) : a - b; }
__device__ __forceinline__ float b3_fma(float a, float b, float c) { return B3_UNPACK_F32 ? fma1(a, b, c) : fmaf(a, b, c); }
__device__ __forceinline__ float b3_mul(float a, float b) { return B3_UNPACK_F32 ? mul1(a, b) : mul_rn(a, b); }   // never contracted

__device__ __forceinline__ float4 b3_scale4(float4 v, float4 s) {          // the per-(sample, channel) modulation scale of four activations
    return make_float4(b3_mul(v.x, s.x), b3_mul(v.y, s.y), b3_mul(v.z, s.z), b3_mul(v.w, s.w));
}

// exact three-way split of four f32 into packed bf16 planes
struct Split4 { uint2 p[3]; };
__device__ __forceinline__ void split2(float a, float b, unsigned& h, unsigned& m, unsigned& l) {
    h = ideas_pk_bf16(a, b);
    const float ra = b3_sub(a, ideas_bf_lo(h)), rb = b3_sub(b, ideas_bf_hi(h));
    m = ideas_pk_bf16(ra, rb);
    l = ideas_pk_bf16(b3_sub(ra, ideas_bf_lo(m)), b3_sub(rb, ideas_bf_hi(m)));   // exact: <= 8 significant bits are left
}
// the same from doubles (operands that are sums of f32 values, e.g. Winograd-transformed weights): the residuals are carried in
// double, so the three planes hold the leading ~26 bits of the EXACT value instead of those of its f32 rounding
__device__ __forceinline__ void split2d(double a, double b, unsigned& h, unsigned& m, unsigned& l) {
    h = ideas_pk_bf16((float)a, (float)b);
    const double ra = a - (double)ideas_bf_lo(h), rb = b - (double)ideas_bf_hi(h);
    m = ideas_pk_bf16((float)ra, (float)rb);
    l = ideas_pk_bf16((float)(ra - (double)ideas_bf_lo(m)), (float)(rb - (double)ideas_bf_hi(m)));
}
__device__ __forceinline__ Split4 split4(float4 v) {
    Split4 s;
    split2(v.x, v.y, s.p[0].x, s.p[1].x, s.p[2].x);
    split2(v.z, v.w, s.p[0].y, s.p[1].y, s.p[2].y);
    return s;
}

// (bit_cast the WHOLE result: indexing the builtin's return value element-wise makes the optimizer shrink the load to
// one dword and splat it)
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 buffer_load4(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    const f32x4 f = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0));
    return make_float4(f.x, f.y, f.z, f.w);
}

// Byte offsets into the two swizzled LDS layouts of the b3 kernels.
// pix_off: 32-byte rows (16 bf16 of one pixel / slot), the 16-byte half XOR-ed with bit 3 of the row.
__device__ __forceinline__ int pix_off(int pix, int half) { return pix * ROWB + ((half ^ ((pix >> 3) & 1)) << 4); }
// chunk_off: 128-byte rows of eight 16-byte chunks, the chunk XOR-swizzled (by 4) with bit 1 of the row.
__device__ __forceinline__ int chunk_off(int r, int c) { return (r * 8 + (c ^ (((r >> 1) & 1) << 2))) * 16; }

// plane pairs, smallest terms first
constexpr int PA[6] = {2, 0, 1, 1, 0, 0};
constexpr int PB[6] = {0, 2, 1, 0, 1, 0};

}  // namespace
