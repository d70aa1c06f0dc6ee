// The epilogue of the forward-family convolution kernels, said once per precision.
//
// Every kernel ends with the same arithmetic on its accumulator:
//     v = acc * gain;  v *= out_scale[b][n];  v += bias[n];  v = lrelu(v, alpha) * act_gain;  v = (v + resid) * resid_gain;  y (+)= v
// and the bitwise tests of the project (fused == unfused, flat GEMM == generic kernel, LDS-image kernel == generic kernel, fast
// Winograd tails == generic tail) rest on the roundings of that chain being identical at every site.  The kernels call the pieces
// below; none of them writes the chain out itself.
//   f32 rule  (epi_*):      every operation rounded on its own -- bitwise conv -> fused_bias_act -> residual add of the unfused ops.
//   bf16 rule (epi_bf16):   ONE fused multiply-add for out_scale and bias, everything else rounded on its own.
// `P` is anything with the fields gain / act / alpha / act_gain / resid_gain: ideas_conv_params, or EpiScalars in the kernels that
// take the scalars as arguments.  Only mul_rn / mul_then_add / fmaf under contract(off) here: accumulators come from MFMAs, where
// the single-issue helpers of common.hpp (sub1 / mul1 / fma1) must not be used (see their RESTRICTION).
#pragma once
#include "common.hpp"

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct EpiScalars { float gain; int act; float alpha, act_gain, resid_gain; };

// ---- f32 rule ---------------------------------------------------------------------------------------------------------------------
// The loads stay with the caller's control flow: the out_scale value is read HERE, behind the test of the pointer (a value passed as
// `out_scale ? out_scale[i] : 1.f` hoists the load out of the branch and reschedules the whole kernel); the *_val forms are for the
// sites that read one scale per lane ahead of their loop.
template <class P> __device__ __forceinline__ float epi_scale(float acc, const P& p, const float* out_scale, int64_t idx) {
    float v = mul_rn(acc, p.gain);
    if (out_scale) v = mul_rn(v, out_scale[idx]);
    return v;
}
template <class P> __device__ __forceinline__ float epi_scale_val(float acc, const P& p, bool scaled, float os) {
    float v = mul_rn(acc, p.gain);
    if (scaled) v = mul_rn(v, os);
    return v;
}
template <class P> __device__ __forceinline__ float epi_bias_act(float v, const P& p, float bias) {
    v = mul_then_add(v, 1.0f, bias);
    if (p.act) v = (v > 0.f ? v : v * p.alpha) * p.act_gain;
    return v;
}
// head = scale, bias, activation
template <class P> __device__ __forceinline__ float epi_head(float acc, const P& p, const float* out_scale, int64_t idx, float bias) {
    return epi_bias_act(epi_scale(acc, p, out_scale, idx), p, bias);
}
template <class P> __device__ __forceinline__ float epi_head_val(float acc, const P& p, bool scaled, float os, float bias) {
    return epi_bias_act(epi_scale_val(acc, p, scaled, os), p, bias);
}
template <class P> __device__ __forceinline__ float epi_head(float acc, const P& p, float bias) {      // no per-sample scale
    return epi_bias_act(mul_rn(acc, p.gain), p, bias);
}
// tail = residual merge, then the store or the accumulation into y (any storage type of common.hpp's ld1 / st1)
template <class P> __device__ __forceinline__ float epi_resid(float v, float r, const P& p) { return (v + r) * p.resid_gain; }
template <class T> __device__ __forceinline__ void epi_store(T* y, int64_t i, float v, int accumulate) {
    if (accumulate) st1(y + i, ld1(y + i) + v); else st1(y + i, v);
}

// ---------------------------------------------------------------------------------------------------------------
// Branch-free Winograd tails for the epilogue configurations the training step actually launches (conv_b3_wino.hip).  Its generic
// tail tests five run-time flags per channel quad (out_scale / bias / act / resid / accumulate): uniform branches, but each one ends a
// basic block, so its loads are waited for one by one and nothing is packed -- ~600 of a wave's ~1550 vector instructions per 8-chunk
// tile, executed with the matrix pipe idle.  Here the configuration is a template parameter chosen by ONE
// uniform switch per half tile, a thread finishes its 8 channels x 2 pixels in straight-line code on 4-wide vectors (v_pk_add /
// v_pk_mul) from the four inverse-transform components at ex + k * CS, and the four stores take 32-bit buffer offsets.
//   OS: per-(sample, channel) output scale   BA: bias + leaky-ReLU * act_gain   RS: (v + resid) * resid_gain
// A different program from epi_head / epi_resid, with the same op order and no contraction: bitwise equal to them PROVIDED
// 0 <= alpha <= 1, where max(t, alpha t) is the select (t > 0 ? t : alpha t) -- the only slopes the dispatch admits to it
// (tests/test_ops_gpu.py::test_winograd_fast_epilogues_are_bitwise_the_generic_tail).
// ---------------------------------------------------------------------------------------------------------------
typedef float v4f __attribute__((ext_vector_type(4)));
template <bool OS, bool BA, bool RS, int CS>
__device__ __forceinline__ void wino_finish_fast(__amdgpu_buffer_rsrc_t ry, unsigned yoff, unsigned px_step, const float* __restrict__ resid,
                                                 const float* __restrict__ os_p, const float* __restrict__ bias_p,
                                                 const float* __restrict__ ex, bool two, float gain, float alpha, float act_gain,
                                                 float resid_gain) {
#pragma clang fp contract(off)
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        if (g == 1 && !two) break;
        const v4f m0 = *reinterpret_cast<const v4f*>(ex + g * 4 + 0 * CS);
        const v4f m1 = *reinterpret_cast<const v4f*>(ex + g * 4 + 1 * CS);
        const v4f m2 = *reinterpret_cast<const v4f*>(ex + g * 4 + 2 * CS);
        const v4f m3 = *reinterpret_cast<const v4f*>(ex + g * 4 + 3 * CS);
        v4f osv, bv, r0, r1;
        if (OS) osv = *reinterpret_cast<const v4f*>(os_p + g * 4);
        if (BA) bv = *reinterpret_cast<const v4f*>(bias_p + g * 4);
        if (RS) {
            r0 = *reinterpret_cast<const v4f*>(resid + (yoff >> 2) + g * 4);
            r1 = *reinterpret_cast<const v4f*>(resid + ((yoff + px_step) >> 2) + g * 4);
        }
        v4f t0 = (m0 + m1) + m2, t1 = (m1 - m2) - m3;
        t0 = t0 * gain; t1 = t1 * gain;
        if (OS) { t0 = t0 * osv; t1 = t1 * osv; }
        if (BA) {
            t0 = t0 + bv; t1 = t1 + bv;
            const v4f a0 = t0 * alpha, a1 = t1 * alpha;
            t0 = __builtin_elementwise_max(t0, a0) * act_gain;
            t1 = __builtin_elementwise_max(t1, a1) * act_gain;
        }
        if (RS) { t0 = (t0 + r0) * resid_gain; t1 = (t1 + r1) * resid_gain; }
        // (no SGPR offset on the stores: conv_b3_s2fir.hip records the data hazard of the `soffset` form on this part)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned, t0), ry,
                                               (int)(yoff + g * 16), 0, 0);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned, t1), ry,
                                               (int)(yoff + px_step + g * 16), 0, 0);
    }
}

// ---- bf16 rule --------------------------------------------------------------------------------------------------------------------
// As the compiler contracted conv_bf16_kernel's `acc * gain * os + bias` before the roundings were written out: the product with the
// gain is rounded, out_scale and bias are ONE fma, and nothing else is fused.  With os = 1 the fma is exactly mul_then_add(acc,
// gain, bias), which is how the flat 1x1 kernel (no per-sample scale) is bitwise the generic one.
// BIAS = false is the one deviating site, conv_bf16_multi_kernel, left as the parent compiled it: it passes `bias = nullptr` as a
// compile-time constant, and there the compiler did NOT contract -- two rounded products and `+ 0` (which turns a -0 into +0).
// fma(t, os, +0) would equal that except where t * os underflows to zero, whose sign the fma keeps; so the site keeps its own form.
template <bool BIAS = true, class P>
__device__ __forceinline__ float epi_bf16(float acc, const P& p, float os, float bias, bool merge, float r, bool accumulate, float prev) {
#pragma clang fp contract(off)
    float u = BIAS ? fmaf(acc * p.gain, os, bias) : acc * p.gain * os + 0.f;
    if (p.act) u = (u > 0.f ? u : u * p.alpha) * p.act_gain;
    if (merge) u = (u + r) * p.resid_gain;
    if (accumulate) u = u + prev;
    return u;
}

// ---- pieces of the bf16 kernels' tile epilogue (conv_bf16.hip, conv_bf16_pw.hip) ----------------------------------------------------
#define LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))

// The wait in front of a K-step's raw barrier: this wave's DMA pieces of the step have landed (counted vmcnt) AND its LDS reads of
// the previous step have returned.  The second half matters: hipcc floats `s_barrier` (and a bare vmcnt wait) up over the previous
// step's last MFMAs and over the `s_waitcnt lgkmcnt` in front of them, so a wave passed the barrier with ds_reads of stage t-1 still
// queued -- and behind the barrier the other waves' DMA overwrites exactly that stage.  Alone the reads always won that race; next
// to a kernel that keeps the LDS busy (the f32 split weight gradient on the side stream) the image kernel returned a few output
// channels off by one K-step in 20 % of its launches (tools/probes/img_vs_b3wgrad.py; cdna_hip_programming.md: "raw s_barrier +
// lgkmcnt(0)").
template <int N> __device__ __forceinline__ void wait_step() {
    static_assert(N >= 0 && N <= 63, "vmcnt immediate");
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
}

// Register-only widening of the epilogue stores.  In the accumulator layout lane (li, lh) holds, per 32-channel block, the four
// channel quads 8g + 4lh .. +3 (g = 0..3) of pixel li: 8-byte stores, 64 pieces per instruction.  v_permlane32_swap exchanges
// lanes li and li + 32 (the two halves of the SAME pixel): swapping quad g of the upper half with quad g + 2 of the lower half
// leaves lane (li, 0) with channels 0-15 and lane (li, 1) with channels 16-31 of the block -- two 16-byte stores per lane, 32
// contiguous bytes, half the store instructions, no LDS.  out[c] = channels 8 (c + 2 lh) .. + 7 of the block.  With the stores compiled
// out the 128-channel image kernel runs 1030 instead of 750 TFLOP/s at 256x256; this form recovers 820 (Dreal.1.conv1 710 -> 780,
// E.2.conv1 575 -> 840).  (The tile through LDS as whole pixel rows, 128-byte lines per pixel, was the same speed.)
__device__ __forceinline__ void quad_exchange(const uint2 (&q)[4], uint4 (&out)[2]) {
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const auto rx = __builtin_amdgcn_permlane32_swap(q[g].x, q[g + 2].x, false, false);
        const auto ry = __builtin_amdgcn_permlane32_swap(q[g].y, q[g + 2].y, false, false);
        out[g] = make_uint4(rx[0], ry[0], rx[1], ry[1]);
    }
}

// The tile epilogue of conv_bf16_body / conv_bf16_img_kernel.  Lane (li, lh) holds pixel li of row block a; registers 4g .. 4g+3
// of acc[a][b] = channels n0 + 32 (wn NT + b) + 8g + 4lh .. + 3.  `row(a, off, bimg)` looks the lane's pixel up: `off` = its element
// offset in y / resid (MASKED: -1 = a row past the end, nothing loaded or stored), `bimg` = its sample (the row of out_scale).
// BIAS = false: epi_bf16's form for a launch that never has a bias (`bias` is then nullptr).  Cout % 4 == 0; with Cout % 8 == 0 and a 16-byte aligned y the quads are widened to 16-byte stores (quad_exchange).
template <bool MASKED, bool BIAS, int MT, int NT, class RowFn>
__device__ __forceinline__ void bf16_store_tile(ideas_bf16* __restrict__ y, const ideas_bf16* __restrict__ resid,
                                                const float* __restrict__ out_scale, const float* __restrict__ bias,
                                                const ideas_conv_params& p, const f32x16 (&acc)[MT][NT], RowFn row, int n0, int wn, int lh) {
    const bool wide = (p.Cout & 7) == 0 && (((uintptr_t)y) & 15) == 0;      // 16-byte stores after a lane exchange (quad_exchange)
#pragma unroll
    for (int a = 0; a < MT; ++a) {
        int64_t off;
        int bimg;
        row(a, off, bimg);
#pragma unroll
        for (int b = 0; b < NT; ++b) {
            uint2 q[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                q[g] = make_uint2(0u, 0u);
                const int n = n0 + (wn * NT + b) * 32 + 8 * g + 4 * lh;
                if ((MASKED && off < 0) || n >= p.Cout) continue;           // Cout % 4 == 0
                float v[4];
                const float4 bv = bias ? *reinterpret_cast<const float4*>(bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
                const float4 os = out_scale ? *reinterpret_cast<const float4*>(out_scale + (int64_t)bimg * p.Cout + n)
                                            : make_float4(1.f, 1.f, 1.f, 1.f);
                const float bvv[4] = {bv.x, bv.y, bv.z, bv.w}, osv[4] = {os.x, os.y, os.z, os.w};
                uint2 rr = make_uint2(0u, 0u);
                if (resid) rr = *reinterpret_cast<const uint2*>(resid + off + n);
                const float rv[4] = {ideas_bf_lo(rr.x), ideas_bf_hi(rr.x), ideas_bf_lo(rr.y), ideas_bf_hi(rr.y)};
                uint2 prev = make_uint2(0u, 0u);
                if (p.accumulate) prev = *reinterpret_cast<const uint2*>(y + off + n);
                const float pv[4] = {ideas_bf_lo(prev.x), ideas_bf_hi(prev.x), ideas_bf_lo(prev.y), ideas_bf_hi(prev.y)};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    v[j] = epi_bf16<BIAS>(acc[a][b][4 * g + j], p, osv[j], bvv[j], resid != nullptr, rv[j], p.accumulate, pv[j]);
                q[g] = make_uint2(ideas_pk_bf16(v[0], v[1]), ideas_pk_bf16(v[2], v[3]));
                if (!wide) *reinterpret_cast<uint2*>(y + off + n) = q[g];
            }
            if (wide) {                                      // (block-uniform; every lane takes part in the exchange)
                uint4 ch[2];
                quad_exchange(q, ch);
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int n = n0 + (wn * NT + b) * 32 + 8 * (c + 2 * lh);
                    if (!(MASKED && off < 0) && n < p.Cout) *reinterpret_cast<uint4*>(y + off + n) = ch[c];
                }
            }
        }
    }
}

// ---- the row table of the implicit-GEMM kernels -----------------------------------------------------------------------------------
// Row t of the tile (point m0 + t of the flattened (b, oy, ox) grid) -> element offset of its output pixel (-1 from `mend` on:
// nothing is stored) and its sample index, for the first `rows` threads.  The caller carves the two arrays out of its dead LDS
// stages and puts a __syncthreads() behind the call.
__device__ __forceinline__ void epi_row_table(int64_t* row_off, int* row_b, int t, int rows, int64_t m0, int64_t mend,
                                              const ideas_conv_params& p) {
    if (t < rows) {
        const int64_t m = m0 + t;
        int b = 0;
        int64_t off = -1;
        if (m < mend) {
            const int ox = (int)(m % p.OW);
            const int64_t q = m / p.OW;
            const int oy = (int)(q % p.OH);
            b = (int)(q / p.OH);
            off = (((int64_t)b * p.YH + (oy * p.osy + p.ooy)) * p.YW + (ox * p.osx + p.oox)) * p.Cout;
        }
        row_off[t] = off;
        row_b[t] = b;
    }
}
