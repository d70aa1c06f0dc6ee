/*
 * ideas_hip.h — C ABI of libideas_hip.so, the MI355X (gfx950) kernels behind the IDEAS hot path.
 *
 * Drop-in boundary.  The reference binds two pybind11 modules whose single entry
 * points take/return torch::Tensor:
 *     fused.fused_bias_act(input, bias, refer, act, grad, alpha, scale)      stylegan2/op/fused_bias_act.cpp:11-21
 *     upfirdn2d_op.upfirdn2d(input, kernel, up_x, up_y, down_x, down_y,
 *                            pad_x0, pad_x1, pad_y0, pad_y1)                   stylegan2/op/upfirdn2d.cpp:12-23
 * and leaves every convolution to cuDNN through ATen (stylegan2/model.py:115-121,258,273; models.py:32-38).
 * This library replaces all of them with plain-C entry points:
 *
 *   - raw device pointers, int dims, a dtype/layout enum and a hipStream_t (passed as void*);
 *   - the CALLER allocates every output (so memory stays with its own allocator);
 *   - no global state, no allocation, no host synchronisation: every call only enqueues on `stream`.  The only thing a call reads
 *     besides its arguments is a handful of A/B measurement switches in the process environment, looked up PER CALL (nothing is
 *     cached in the library): IDEAS_B3_WINO2D, IDEAS_B3_TPHASE, IDEAS_B3_WGRAD3, IDEAS_B3_WGRAD3_S2, IDEAS_S2FIR_CFG,
 *     IDEAS_BF16_IMG, IDEAS_BF16_WGRAD3, IDEAS_B3_PW, IDEAS_B3_PW_WGRAD, IDEAS_BF16_PW, IDEAS_B3_WINO_EPI, IDEAS_S2IMG_MIN_BLOCKS,
 *     IDEAS_B3_WINO_N256, IDEAS_BF16_WGRAD3_MIN_WORK -- each "0" selects the older kernel of its family, unset = the default
 *     dispatch; the *_MIN_BLOCKS variable, IDEAS_B3_WINO_N256 and IDEAS_BF16_WGRAD3_MIN_WORK also take a number.
 *     (IDEAS_BF16_WGRAD3_MIN_WORK: the least B * OH * OW * Cin * Cout at which ideas_conv_wgrad(IDEAS_BF16) gives a 3x3 / stride-1
 *     layer to the tap-fused kernel; unset = 6000000000; "0" here admits every shape the kernel's geometry covers, so that tests
 *     reach it at small shapes.  ideas_bf16_wgrad3_supported answers for a shape under the current environment.)
 *     (IDEAS_B3_WINO_N256: "0" keeps the 64 x 128 tile of the row-sharing Winograd kernel where Cout % 256 == 0; a positive number
 *     n replaces the default tile-count rule by "at least n tiles of 64 x 256" (1: wherever Cout allows).  A diagnostic query beside this ABI, defined next to the
 *     dispatch in csrc/conv_b3_wino.hip, tells tests and A/B scripts which tile a forward of a given shape takes.)
 *     What IS memoised per process: immutable device properties (the CU count and the occupancy hipOccupancy... reports for the
 *     library's own split-K kernels), used to size grids -- in one place, csrc/conv_launch.hpp (ideas_cu_count,
 *     ideas_blocks_per_cu), each initialised once and thread-safely;
 *   - return value: 0 = enqueued; negative = argument error (IDEAS_E_*); positive = hipError_t of the launch.
 *
 * Layouts.  IDEAS_NCHW is the reference's layout (bias index (i / inner) % C,
 * fused_bias_act_kernel.cu:29).  IDEAS_NHWC is the MI355X fast path: channels innermost, so bias index is
 * i % C, every load is a coalesced 16-byte vector and the 3x3 contraction's K axis (ky,kx,ci) is contiguous.
 * The convolution entry points are NHWC-only.
 */
#ifndef IDEAS_HIP_H
#define IDEAS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IDEAS_ABI_VERSION 4   /* 2: the per-sample reductions of the modulated-conv backward accumulate in double (round 3);
                                 3: ideas_demod_bwd overwrites dot_d, ideas_weight_prep_batched added;
                                 4: the entry points added since 3 are REQUIRED by the Python binding -- ideas_patch_resize,
                                    ideas_image_u8_to_f32, ideas_stream_create, ideas_linear_fwd / _bwd_x / _bwd_w +
                                    ideas_sizeof_linear_seg (minimum version for the EqualLinear API).  The Python binding
                                    (ideas_amd/_lib.py) requires `ideas_abi_version() == 4` EXACTLY, before it looks any symbol
                                    up: a library of another version, older or newer, is refused.  Version 4 also REMOVED
                                    ideas_b3_wino_wgrad_supported and the IDEAS_F32_B3 form of ideas_conv3x3_wino_wgrad.
                                    Entry points marked "additive within ABI 4" below came later without a bump: the binding
                                    looks every one of them up, so a version-4 library built before one of them fails there
                                    with the missing symbol's name. */

enum { IDEAS_NCHW = 0, IDEAS_NHWC = 1 };
/* `dtype` of the convolution entry points.  Tensors are f32 in HBM for both values.
 *   IDEAS_F32     contraction on the f32 matrix instruction (v_mfma_f32_32x32x2_f32): an exact fmaf chain.
 *   IDEAS_F32_B3  operands split exactly into three bf16 planes, six plane-pair products on the bf16 matrix
 *                 instruction with f32 accumulation (csrc/conv_b3.hip): the same f32 error class at 2.67x the matrix
 *                 rate.  Shapes the split kernels do not cover (Cin % 16 != 0) run the IDEAS_F32 kernel.
 *   IDEAS_BF16    bf16 mixed precision (BASELINE.json configs[4]; the reference's ops dispatch half as well,
 *                 fused_bias_act_kernel.cu:78, upfirdn2d_kernel.cu:311): activations (x, y, gy, resid) are bf16 in HBM,
 *                 contraction on v_mfma_f32_32x32x16_bf16 with f32 accumulation and an f32 epilogue; weights stay f32 masters
 *                 (the MFMA kernels read a bf16 pack of them, ideas_bf16_pack_weights), scales / biases / weight gradients f32.
 * Two more values are taken ONLY by ideas_fused_bias_act and ideas_upfirdn2d (the reference's ops dispatch float, double and half,
 * fused_bias_act_kernel.cu:78, upfirdn2d_kernel.cu:311); every other entry point returns IDEAS_E_UNSUPPORTED for them:
 *   IDEAS_F16     half activations (_Float16 in HBM), f32 arithmetic, one rounding to half at the store.
 *   IDEAS_F64     double activations and double arithmetic; the f32 side arguments of those two calls (bias, bias_grad, fir) are
 *                 then double as well -- the pointer is passed through as the element type the dtype names.
 * (Additive within ABI 4: no signature changed; an older library answers IDEAS_E_UNSUPPORTED.) */
enum { IDEAS_F32 = 0, IDEAS_F32_B3 = 1, IDEAS_BF16 = 2, IDEAS_F16 = 3, IDEAS_F64 = 4 };

enum {
    IDEAS_OK = 0,
    IDEAS_E_NULL = -1,      /* a required pointer is NULL                 */
    IDEAS_E_SHAPE = -2,     /* a dimension is <= 0 or inconsistent        */
    IDEAS_E_UNSUPPORTED = -3, /* dtype / layout / mode not implemented   */
    IDEAS_E_ALIGN = -4      /* pointer or channel count not 16-B aligned where the kernel needs it */
};

int ideas_abi_version(void);
int ideas_sizeof_conv_params(void);   /* lets a binding check its mirror of ideas_conv_params */
const char* ideas_strerror(int code);

/* Stream helper (no reference counterpart: the reference runs everything on torch's current stream).  Creates a non-blocking HIP
 * stream of the lowest (prio < 0), default (prio == 0) or highest (prio > 0) priority of the device; the caller owns it
 * (ideas_stream_destroy).  The host side runs the weight-gradient kernels on a lowest-priority stream so that they fill what the
 * input-gradient chain on the caller's stream leaves free instead of competing with it for compute units. */
int ideas_stream_create(void** out_stream, int prio);
int ideas_stream_destroy(void* stream);

/* ------------------------------------------------------------------------------------------------
 * fused bias + leaky-ReLU.  Replaces fused_bias_act_op (fused_bias_act_kernel.cu:52-98).
 *
 *   v   = x[i] + (b ? b[channel(i)] : 0)
 *   y   = (grad == 0) ?  (v   > 0 ? v : v * alpha) * scale            -- act=3, grad=0  (forward)
 *       : (grad == 1) ?  (ref > 0 ? v : v * alpha) * scale            -- act=3, grad=1  (backward / grad-grad)
 *       :                0                                            -- grad == 2
 *   act == 1 is the linear variant (y = v * scale; 0 for grad == 2).
 *
 * `n` = total elements, `C` = channels, `inner` = product of dims after the channel dim (NCHW only; a
 * [B,C] matrix is inner = 1).  `ref` is required iff grad == 1.  `bias_grad` (optional, grad == 1 only):
 * if non-NULL it must be a ZEROED float[C]; the kernel adds sum over (n,h,w) of y into it, fusing the
 * reference's separate grad_input.sum(dim) pass (fused_act.py:33-38).
 * dtypes: IDEAS_F32 and IDEAS_F16 (x, y, ref half; b, bias_grad f32; f32 arithmetic in act's operation order, rounded once at the
 * store) in NCHW, NHWC and [B,C]; IDEAS_BF16 in NHWC and [B,C]; IDEAS_F64 in all three, with x, y, ref, b AND bias_grad double
 * (`bias_grad` is then a double* passed as float*).  `alpha` / `scale` are float for every dtype (the reference's binding takes
 * float alpha, scale, fused_bias_act.cpp:12, and widens them).
 * ---------------------------------------------------------------------------------------------- */
int ideas_fused_bias_act(void* y, const void* x, const void* b, const void* ref, float* bias_grad,
                         int64_t n, int C, int64_t inner, int layout,
                         int act, int grad, float alpha, float scale, int dtype, void* stream);

/* Per-channel sum of a channels-innermost tensor (x: n elements, NHWC or [B,C]; any C <= 8192): out[c] (+)= sum of x[.., c].
 * The gradient of a plain conv bias (EqualConv2d with bias and no activation = G.to_rgb, stylegan2/model.py:94-123,
 * models.py:120), which autograd takes as grad.sum((0, 2, 3)).  `clear` != 0 zeroes out[0..C) first.  (additive since ABI 3.) */
int ideas_channel_sum(float* out, const void* x, int64_t n, int C, int clear, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * upfirdn2d.  Replaces upfirdn2d_op (upfirdn2d_kernel.cu:209-368): zero-stuff by `up`, pad (negative pad
 * crops), correlate with the FLIPPED kh x kw FIR, decimate by `down`.  x is [B,C,in_h,in_w] (NCHW) or
 * [B,in_h,in_w,C] (NHWC); y has out = (in*up + pad0 + pad1 - k) / down + 1 per axis.  `fir` is a device
 * float[kh*kw], row-major, any kh, kw >= 1 (tables too large for LDS are read from global memory).  `gain` multiplies the FIR
 * (1.0f for the plain op).  dtypes: IDEAS_F32 and IDEAS_F16 (f32 FIR, f32 accumulation) in both layouts, IDEAS_BF16 in NHWC,
 * IDEAS_F64 in both layouts with `fir` a device double[kh*kw] (passed as float*) and double accumulation.
 * The gradient is the same call with up<->down swapped, the FIR flipped and
 * pads (k - p0 - 1, in*up - out*down + p0 - up + 1)  (upfirdn2d.py:111-114).
 * ---------------------------------------------------------------------------------------------- */
int ideas_upfirdn2d(void* y, const void* x, const float* fir,
                    int B, int C, int in_h, int in_w, int out_h, int out_w,
                    int kh, int kw, int up_x, int up_y, int down_x, int down_y,
                    int pad_x0, int pad_y0, float gain, int flip,
                    int layout, int dtype, void* stream);

/* The 4x4 NHWC blur (up = down = 1; C % 4 == 0) with the elementwise pass that always follows it on the IDEAS path folded into
 * its store, so the blurred tensor is never written and read back:
 *   mode 1 (IDEAS_BLUR_ACT_BWD):  y = (ref > 0 ? v : v*alpha) * scale,  bias_grad[c] += sum over (b,h,w) of y
 *        v = the blur of x.  The gradient of a downsampling ConvLayer's Blur (models.py:69, upfirdn2d.py:19-45) followed by the
 *        leaky-ReLU backward of the conv layer below it (fused_act.py:20-47); `ref` = that layer's saved output, same shape and
 *        dtype as y; `bias_grad` float[C], accumulated into (not zeroed here).
 *   mode 2 (IDEAS_BLUR_BIAS_ACT): y = lrelu(v + bias[c], alpha) * scale
 *        the Blur of an upsampling ModulatedConv2d followed by its FusedLeakyReLU (stylegan2/model.py:258-261, 371-377).
 * Operation order is that of ideas_upfirdn2d -> ideas_fused_bias_act (for bf16 the blur is rounded to bf16 in between, as the
 * two-kernel path stores it), so f32 results are bitwise the unfused ones.  `flip` / `gain` / pads as in ideas_upfirdn2d. */
/* The zero-stuffing 4x4 NHWC FIR (up = 2, down = 1; C % 4 == 0) of ideas_upfirdn2d plus a tensor of the output's shape:
 * y = fir(x) + resid.  Forward: the residual merge behind an upsampling skip branch (models.py:160-178: (conv2(...) + skip) with
 * the skip ending in a Blur); backward: the sum of the two input gradients of a downsampling ResBlock, whose skip branch starts
 * with the decimating FIR this kernel is the adjoint of.  Saves the separate add pass (3 tensor passes). */
int ideas_fir_up2_add(void* y, const void* x, const float* fir, const void* resid, int B, int C, int in_h, int in_w, int out_h,
                      int out_w, int pad_x0, int pad_y0, float gain, int flip, int dtype, void* stream);

#define IDEAS_BLUR_ACT_BWD 1
#define IDEAS_BLUR_BIAS_ACT 2
int ideas_blur_fused(void* y, const void* x, const float* fir, int B, int C, int in_h, int in_w, int out_h, int out_w,
                     int pad_x0, int pad_y0, float gain, int flip, int mode, const void* ref, const float* bias,
                     float* bias_grad, float alpha, float scale, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution on the f32 MFMA pipe (v_mfma_f32_32x32x2_f32), NHWC.
 * Replaces the cuDNN calls behind F.conv2d / F.conv_transpose2d (stylegan2/model.py:115-121,258,273;
 * models.py:32-38) and, with in_scale/out_scale, the per-sample weight materialisation of
 * ModulatedConv2d (stylegan2/model.py:240-248):  y[b,:,:,o] = out_scale[b,o] * sum w[o,t,i] * in_scale[b,i] * x[b,..,i].
 *
 * One launch computes, for every point (b, oy, ox) of a logical OH x OW grid and every output channel o:
 *     acc = sum over taps (ty,tx) in [0,TY)x[0,TX) and ci in [0,Cin) of
 *              wmat[o][(ty*TX+tx)*Cin + ci] * X(b, oy*sy + ty*dy + offy, ox*sx + tx*dx + offx, ci)
 *     where X(...) is 0 outside [0,IH)x[0,IW) (or mirrored, reflect=1), times in_scale[b*Cin+ci] if given;
 *     y[b, oy*osy + ooy, ox*osx + oox, o] = epilogue(acc)
 * The output tensor is [B, YH, YW, Cout].  This one parameterisation covers forward convs (sy = stride,
 * dy = 1, off = -pad), input gradients of stride-1 convs (flipped/transposed wmat), and the four parity
 * phases of stride-2 transposed convs / stride-2 input gradients (osy = 2, ooy = phase).
 *
 * epilogue(acc): v = acc * gain * (out_scale ? out_scale[b*Cout+o] : 1) + (bias ? bias[o] : 0);
 *                if act: v = (v > 0 ? v : v*alpha) * act_gain;
 *                if resid: v = (v + resid[same index as y]) * resid_gain;
 *                if accumulate: y += v else y = v.
 * Requires Cin % 4 == 0 and 16-byte aligned x / wmat.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ideas_conv_params {
    int B, IH, IW, Cin;          /* input  [B,IH,IW,Cin]                    */
    int YH, YW, Cout;            /* output tensor [B,YH,YW,Cout]            */
    int OH, OW;                  /* logical grid computed by this launch    */
    int TY, TX;                  /* taps                                    */
    int sy, sx, dy, dx, offy, offx;
    int osy, osx, ooy, oox;      /* output placement                        */
    int reflect;                 /* 1 = mirror out-of-range input coords    */
    int act;                     /* 1 = leaky-ReLU epilogue                 */
    float alpha, act_gain, resid_gain;
    int accumulate;
    float gain;                  /* uniform multiplier on the accumulator (equalised-lr weight scale) */
} ideas_conv_params;

int ideas_conv_igemm(void* y, const void* x, const void* wmat, const float* in_scale, const float* out_scale,
                     const float* bias, const void* resid, const ideas_conv_params* p, int dtype, void* stream);

/* Split-bf16 ("b3") operand preparation for dtype IDEAS_F32_B3 (kernels: csrc/conv_b3.hip; preparation: csrc/weight_prep.hip).
 *   ideas_b3_conv_supported  1 if ideas_conv_igemm(..., IDEAS_F32_B3, ...) covers the geometry (Cin % 16 == 0, <= 32 taps,
 *                            x and the weight planes < 4 GiB: the kernel addresses them with 32-bit buffer offsets).
 *   ideas_b3_split_weights   wmat f32 [Cout][K] (the same matrix ideas_conv_igemm takes for IDEAS_F32) -> `planes`,
 *                            3*Cout*K bf16 laid out [3][K/16][Cout][16] with the K-steps
 *                            ordered (ci/16, ty, tx); K = taps*Cin, Cin % 16 == 0.  With IDEAS_F32_B3 the `wmat`
 *                            argument of ideas_conv_igemm is this buffer.  Activations are split inside the kernel. */
int ideas_b3_conv_supported(const ideas_conv_params* p);
int ideas_b3_wgrad_supported(const ideas_conv_params* p);   /* 1 if ideas_conv_wgrad(IDEAS_F32_B3) runs the split kernel; otherwise it
                                                                runs the IDEAS_F32 kernel (same arguments, same result class) */
int ideas_b3_wgrad3_supported(const ideas_conv_params* p);  /* 1 if that split weight gradient is the tap-fused 3x3 kernel with a rolling
                                                                activation window (csrc/conv_b3_wgrad3.hip: 3x3, stride 1 or 2,
                                                                OW % 16 == 0, Cin % 64 == 0, Cout % 64 == 0); informational */
int ideas_b3_split_weights(void* planes, const void* wmat, int Cout, int K, int Cin, void* stream);
/* The same planes read straight from a parameter of any strides: element (n, ty, tx, ci) of the launch's weight matrix is
 * w[n*sn + ty*sty + tx*stx + ci*sc] (floats; w already points at the first element).  Covers the forward matrix of an
 * [O,I,KH,KW] tensor in either memory format, the phase-sliced transposed matrix of an input gradient (tap step = the conv
 * stride) and the matrix of a transposed conv, without materialising a permuted / sliced f32 copy first. */
int ideas_b3_split_weights_strided(void* planes, const float* w, int Cout, int TY, int TX, int Cin, int64_t sn, int64_t sty,
                                   int64_t stx, int64_t sc, void* stream);
/* The same for ideas_conv3x3_wino(IDEAS_F32_B3): Winograd-transformed AND split weights, 12*N*3*C bf16 laid out
 * [4 v][3 planes][3*C/16 steps][N][16] (step = (c/16)*3 + ky).  Element (n, ky, kx, c) of the 3x3 kernel is read at
 * w[base + n*sn + ky*sky + kx*skx + c*sc] (floats), so the forward matrix (n = o, c = i) and the flipped / transposed one
 * of the input gradient (n = i, c = o) both come straight from the OHWI parameter. */
int ideas_b3_wino_supported(const ideas_conv_params* p);
int ideas_b3_wino_split_weights(void* planes, const void* w, int N, int C, int64_t sn, int64_t sky, int64_t skx, int64_t sc,
                                int64_t base, void* stream);

/* bf16 mixed precision (dtype IDEAS_BF16 of ideas_conv_igemm / ideas_conv_wgrad; csrc/conv_bf16.hip, the pack: csrc/weight_prep.hip).
 *   ideas_bf16_conv_supported   1 if ideas_conv_igemm(..., IDEAS_BF16, ...) covers the geometry: Cin % 32 == 0, Cout % 4 == 0,
 *                               <= 32 taps, tensors < 4 GiB (`scaled`: an in_scale will be passed; M tiles are then cut per sample
 *                               and the block scales its weight tile by in_scale[b, :]).
 *   ideas_bf16_wgrad_supported  the same for ideas_conv_wgrad: Cin % 8 == 0, Cout % 8 == 0, OW a divisor or a multiple of 32.
 *   ideas_bf16_pack_weights     wmat f32 [Cout][K] (K = taps*Cin, the matrix ideas_conv_igemm takes for IDEAS_F32) -> `pack`,
 *                               Cout*K bf16 laid out [K/32][Cout][32], K-steps ordered (ci/32, ty, tx), 16-byte chunk c of row
 *                               n stored at position c ^ ((n >> 2) & 3) (the LDS swizzle, so the kernel's DMA is linear).
 *                               in_scale == NULL: one pack (B must be 1).  in_scale = float[B][Cin] (modulated conv): B packs,
 *                               pack b = bf16(w[n][k] * in_scale[b][ci(k)]) -- the reference's per-sample weights
 *                               (stylegan2/model.py:240-248) for the life of one launch.
 *                               With IDEAS_BF16 the `wmat` argument of ideas_conv_igemm is this buffer; pass the same in_scale
 *                               to ideas_conv_igemm (it selects the per-sample packs; the scale itself is already applied). */
int ideas_bf16_conv_supported(const ideas_conv_params* p, int scaled);
int ideas_bf16_wgrad_supported(const ideas_conv_params* p, int scaled);
int ideas_bf16_wgrad3_supported(const ideas_conv_params* p);   /* 1 exactly when ideas_conv_wgrad(IDEAS_BF16) launches the tap-fused 3x3
                                                                   kernel for *p under the current environment (3x3, unit stride and
                                                                   dilation, offsets -2 .. 0, OW % 32 == 0, OH >= 8, Cin % 64 == 0,
                                                                   Cout % 64 == 0, IDEAS_BF16_WGRAD3 not "0", B * OH * OW * Cin * Cout
                                                                   >= IDEAS_BF16_WGRAD3_MIN_WORK); the launcher asks this function.
                                                                   Informational; additive within ABI 4 */
/* (A diagnostic query beside this ABI, defined next to the dispatch in csrc/conv_bf16.hip, tells tests and A/B scripts which forward
 * tile -- 256 x 128 on 8 waves, 128 x 128, 128 x 64 or 128 x 32 -- a launch of a given shape takes, and whether the LDS-image kernel
 * takes it first.) */
int ideas_bf16_pack_weights(void* pack, const void* wmat, const float* in_scale, int B, int Cout, int K, int Cin, void* stream);
/* ideas_bf16_pack_weights reading the matrix through strides (see ideas_b3_split_weights_strided). */
int ideas_bf16_pack_weights_strided(void* pack, const float* w, const float* in_scale, int B, int Cout, int TY, int TX, int Cin,
                                    int64_t sn, int64_t sty, int64_t stx, int64_t sc, void* stream);
/* The three derived-weight forms above as ONE kind of job (csrc/weight_prep.hip): an ideas_prep_desc names the destination, the first
 * element of the matrix, its dims and its strides in floats.  The entry points above fill one and take the same path.
 *   IDEAS_PREP_B3_SPLIT   dst = planes of ideas_b3_split_weights_strided(w, Cout=a[0], TY=a[1], TX=a[2], Cin=a[3], s = sn,sty,stx,sc)
 *   IDEAS_PREP_B3_WINO    dst = planes of ideas_b3_wino_split_weights(w, N=a[0], C=a[1], s = sn,sky,skx,sc,base)
 *   IDEAS_PREP_BF16_PACK  dst = pack of ideas_bf16_pack_weights_strided(w, in_scale, B, Cout=a[0], TY=a[1], TX=a[2], Cin=a[3], s = ...)
 * ideas_weight_prep_plan  host arithmetic only, no device call: checks a[] for form `op` (IDEAS_E_SHAPE: a dimension <= 0;
 *                         IDEAS_E_ALIGN: channels a[3] % 16 (split), a[3] % 32 (pack), a[1] % 16 (Winograd)), FILLS d->unit (the
 *                         16-byte read path: s[3] == 1, w 16-byte aligned, s[0..2] multiples of 4; never for the Winograd form) and
 *                         d->nblocks (256-thread blocks of the job) and reports the bf16 elements of the destination (of ONE pack).
 *                         dst and block0 are not read.  This is the only statement of those rules: callers do not restate them.
 * ideas_weight_prep       one job from a HOST descriptor (planned here again: unit / nblocks of the argument are not trusted).
 *                         in_scale / B belong to the pack: float [B][a[3]], 16-byte aligned, B <= 65535 packs of dst_elems each;
 *                         without a scale B must be 1, and the other forms take in_scale == NULL (IDEAS_E_UNSUPPORTED).
 * ideas_weight_prep_batched  MANY planned jobs of one form in one launch (the forms are remade after every optimiser step: one
 *                         launch instead of ~100 small ones per form and network group).  `table` = n descriptors IN DEVICE MEMORY
 *                         (the caller builds them once: parameter and destination addresses do not change between steps), each as
 *                         ideas_weight_prep_plan left it plus dst and block0: block0 / nblocks give each descriptor's share of the
 *                         `total_blocks` blocks (descriptors sorted by block0, first 0, contiguous).  No scale.
 * Per element every route runs the same body: results are bitwise the same.  (Additive within ABI 4: IDEAS_ABI_VERSION stays 4.) */
enum { IDEAS_PREP_B3_SPLIT = 0, IDEAS_PREP_B3_WINO = 1, IDEAS_PREP_BF16_PACK = 2 };
typedef struct ideas_prep_desc {
    void* dst;
    const float* w;
    int64_t s[5];
    int a[4];
    int unit;        /* 1: unit channel stride and 16-byte aligned rows (vector reads); set by ideas_weight_prep_plan */
    int block0;
    int nblocks;     /* set by ideas_weight_prep_plan */
    int pad_;
} ideas_prep_desc;
int ideas_sizeof_prep_desc(void);
int ideas_weight_prep_plan(ideas_prep_desc* d, int op, int64_t* dst_elems);
int ideas_weight_prep(const ideas_prep_desc* host_desc, int op, const float* in_scale, int B, void* stream);
int ideas_weight_prep_batched(const ideas_prep_desc* table, int n, int op, int total_blocks, void* stream);
/* 1 if ideas_conv_direct / ideas_conv_wgrad_direct with IDEAS_BF16 are the intended path for the geometry: the HBM-bound
 * pointwise layers with <= 8 input or output channels (from-RGB, to-RGB and their gradients).  Everything else without a bf16
 * MFMA kernel (a handful of tiny layers) is computed by the caller in f32 on casts. */
int ideas_bf16_direct_supported(const ideas_conv_params* p);

/* Weight gradient of the same family:  for every o, tap, ci
 *     gw[o][(ty*TX+tx)*Cin + ci] (+)= sum over (b,oy,ox) of  G(b,oy,ox,o) * X(b, iy, ix, ci)
 * with G = gy[b, oy*osy+ooy, ox*osx+oox, o] * (out_scale ? out_scale[b*Cout+o] : 1),
 *      X as above (zero / reflect outside, times in_scale).  gw must be ZEROED by the caller unless it is
 * meant to accumulate; split-K partial sums (times `gain`) are added with float atomics (order not
 * deterministic).
 * Requires Cin % 4 == 0 and Cout % 4 == 0.
 */
int ideas_conv_wgrad(float* gw, const void* gy, const void* x, const float* in_scale, const float* out_scale,
                     const ideas_conv_params* p, int dtype, void* stream);

/* 3x3, stride 1, padding 1 (zero or mirrored) convolution through a 1-D Winograd F(2,3) transform along x: four
 * GEMMs with K = 3*Cin instead of one with K = 9*Cin (1.5x fewer MFMAs), same epilogue as ideas_conv_igemm.
 * `umat` = transformed weights [4][Cout][3][Cin]:  U0 = w[..,kx=0], U1 = (w0+w1+w2)/2, U2 = (w0-w1+w2)/2, U3 = w[..,kx=2]
 * (for an input gradient pass the weights flipped in ky,kx with in/out channels swapped).  p must describe the plain
 * geometry (TY = TX = 3, s = 1, OH = IH, OW = IW); requires IW even and Cin % 8 == 0. */
int ideas_conv3x3_wino(void* y, const void* x, const void* umat, const float* in_scale, const float* out_scale,
                       const float* bias, const void* resid, const ideas_conv_params* p, int dtype, void* stream);

/* Weight gradient of the same layers in the Winograd domain: gu (ZEROED float [4][Cout][3][Cin]) receives
 * dU_v = gain * sum dM_v (x) V_v with dM = (g0, g0+g1, g0-g1, -g1); the caller folds it back to the 3x3 taps:
 * dw[kx=0] = dU0 + (dU1+dU2)/2, dw[kx=1] = (dU1-dU2)/2, dw[kx=2] = (dU1+dU2)/2 + dU3.  Cout % 4 == 0 as well. */
int ideas_conv3x3_wino_wgrad(float* gu, const void* gy, const void* x, const float* in_scale, const float* out_scale,
                             const ideas_conv_params* p, int dtype, void* stream);
/* (dtype IDEAS_F32 only: the split-bf16 form of this call, measured no faster than the direct split weight gradient in rounds 2-5,
 * left the library in round 6 -- tools/attic/conv_b3_wino_wgrad.hip.)
 * ideas_wino_wgrad_fold ADDS the folded taps to gw -- element (o, ky, kx, ci) at gw[o*so + ky*sky + kx*skx + ci*sc] (floats), so
 * the OHWI gradient of a parameter or a strided view of a flat gradient bucket -- and, with `clear`, re-zeroes dU behind the
 * read (a persistent scratch then never needs a fill launch).  Replaces the autograd weight gradient of the F.conv2d calls at
 * stylegan2/model.py:115-121 (EqualConv2d) and :262-277 (ModulatedConv2d, same-resolution branch) for the 3x3 layers. */
int ideas_wino_wgrad_fold(float* gw, float* gu, int Cout, int Cin, int64_t so, int64_t sky, int64_t skx, int64_t sc, int clear,
                          void* stream);

/* Up to four launches of ideas_conv_igemm(IDEAS_F32_B3) on ONE tensor pair in one grid: the output-parity phases of a stride-2
 * input gradient / transposed convolution (stylegan2/model.py:250-261, models.py:32-38: the zero-stuffed taps are never multiplied;
 * 4 / 2 / 2 / 1 taps for a 3x3 kernel).  params[i] and wmat[i] (planes of ideas_b3_split_weights) describe launch i; x, y, the
 * per-sample scales, B / IH / IW / Cin / YH / YW / Cout are shared; no bias / resid / act / accumulate / reflect.  The launches run
 * back to back inside one grid, in the order given (put the one with the most taps first): no grid ramp / tail per launch.
 * dtype IDEAS_BF16: the same for the bf16 family, wmat[i] = the packs of ideas_bf16_pack_weights_strided (one per sample when
 * in_scale is given -- only its presence is used, the scale is in the packs).  When the launches are the canonical 3x3 / stride-2
 * / pad-0 phases and Cout > 64, IDEAS_F32_B3 runs them as ONE pass over a shared LDS image of the input (csrc/conv_b3_tphase.hip). */
int ideas_conv_igemm_multi(int n, void* y, const void* x, const void* const* wmat, const float* in_scale, const float* out_scale,
                           const ideas_conv_params* params, int dtype, void* stream);

/* Blur -> 3x3 / stride-2 convolution of a downsampling ConvLayer in ONE kernel (csrc/conv_b3_s2fir.hip, dtype IDEAS_F32_B3 only):
 * replaces upfirdn2d_op(x, kernel, pad) followed by F.conv2d(stride=2) (models.py:68-76 -> stylegan2/model.py:88-91, 115-121) without
 * writing the blurred tensor to HBM: a block builds the blurred pixels under its 8 x 16 output patch in LDS (the separable 4-tap FIR
 * in f32, then the exact 3-way bf16 split) and contracts the nine stride-2 taps from that image.
 *   p        the stride-2 convolution on the BLURRED tensor [B, IH, IW, Cin]: TY = TX = 3, sy = sx = 2, no padding, dense output
 *            (YH = OH = (IH - 3) / 2 + 1); epilogue fields (gain, act, alpha, act_gain, resid_gain) as ideas_conv_igemm;
 *   x        the RAW input [B, xh, xw, Cin] f32 NHWC; IH = xh + pad0 + pad1 - 3 with 0 <= pad0, pad1 <= 3 (the Blur's pads);
 *   fir_h/v  HOST pointers to the 4 + 4 factors of the flipped, gain-scaled FIR: xb[i,j] = sum_a fir_v[a] * (sum_b fir_h[b] *
 *            x[i + a - pad0, j + b - pad0]) -- evaluated in exactly that order with fused multiply-adds, as the stand-alone blur does;
 *   wplanes  the planes of ideas_b3_split_weights for the [Cout][3*3*Cin] matrix; bias / resid optional (float[Cout] / y's shape);
 *   xb_out   optional [B, IH, IW, Cin] f32: the blurred tensor as a side output (the operand of the layer's weight gradient); needs
 *            IH == 2*OH + 1 and IW == 2*OW + 1 (every blurred pixel lies under some output pixel's taps), else IDEAS_E_UNSUPPORTED.
 * ideas_b3_blur_conv_s2_supported: 1 if the geometry is covered (Cin % 16 == 0, Cout % 4 == 0, tensors < 4 GiB). */
int ideas_b3_blur_conv_s2_supported(const ideas_conv_params* p, int xh, int xw, int pad0);
int ideas_b3_blur_conv_s2(void* y, void* xb_out, const void* x, const void* wplanes, const float* fir_h, const float* fir_v,
                          const float* bias, const void* resid, const ideas_conv_params* p, int xh, int xw, int pad0, void* stream);
/* The same kernel for the downsampling ModulatedConv2d (stylegan2/model.py:210-216 Blur, :263-269 F.conv2d(stride=2, groups=batch)) in
 * the re-associated form of ideas_conv_igemm's per-sample scales -- the blur is linear and per channel, so
 *     y[b,o] = epilogue( gain * out_scale[b,o] * sum_{i,k} W[o,i,k] * (in_scale[b,i] * xb[b,i, 2. + k]) ),  xb = the blurred tensor:
 *   in_scale  float[B][Cin] (16-byte aligned), multiplied into the blurred f32 value with ONE rounding before the 3-way split -- the
 *             staged operand is bitwise in_scale * (the stand-alone blur's output), what ideas_conv_igemm(in_scale) stages behind a
 *             blur pass;
 *   out_scale float[B][Cout], multiplied into the accumulator after `gain` and before the bias, as ideas_conv_igemm does;
 *   xb_out    stays the UNSCALED blurred tensor (ideas_conv_wgrad applies in_scale itself).
 * Either scale may be NULL (= 1); with both NULL the result is bitwise that of ideas_b3_blur_conv_s2.  Every other argument, the
 * argument checks and ideas_b3_blur_conv_s2_supported are those of ideas_b3_blur_conv_s2.
 * (Additive within ABI 4: no signature changed; IDEAS_ABI_VERSION stays 4.) */
int ideas_b3_blur_conv_s2_mod(void* y, void* xb_out, const void* x, const void* wplanes, const float* fir_h, const float* fir_v,
                              const float* in_scale, const float* out_scale, const float* bias, const void* resid,
                              const ideas_conv_params* p, int xh, int xw, int pad0, void* stream);

/* Generic direct convolution (VALU) with the same parameterisation and epilogue; any Cin/Cout. Used for the
 * handful of tiny-K layers (RGB / N-channel inputs) where the MFMA tile would be empty. */
/* (dtype IDEAS_F32, or IDEAS_BF16: bf16 x / y / resid / gy with f32 weights, scales, bias and weight gradient) */
int ideas_conv_direct(void* y, const void* x, const void* wmat, const float* in_scale, const float* out_scale,
                      const float* bias, const void* resid, const ideas_conv_params* p, int dtype, void* stream);
int ideas_conv_wgrad_direct(float* gw, const void* gy, const void* x, const float* in_scale, const float* out_scale,
                            const ideas_conv_params* p, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Style demodulation (stylegan2/model.py:243-244):  d[b,o] = rsqrt( sum_i s[b,i]^2 * wsq[o,i] + eps )
 * where wsq[o,i] = scale^2 * sum_k W[o,i,k]^2.  One wavefront per (b,o), shuffle reduction over Cin.
 * ---------------------------------------------------------------------------------------------- */
int ideas_demod(float* d, const float* s, const float* wsq, int B, int Cin, int Cout, float eps, void* stream);
/* wsq[o][i] = scale2 * sum_{ky,kx} W[o][i][ky][kx]^2 of a 4-D f32 weight of strides (so, si, sky, skx) (elements). */
int ideas_weight_sqsum(float* wsq, const float* w, int Cout, int Cin, int KH, int KW, int64_t so, int64_t si, int64_t sky, int64_t skx,
                       float scale2, void* stream);
/* The same table accumulated and stored in double (the operand of ideas_demod_bwd). */
int ideas_weight_sqsum_f64(double* wsq, const float* w, int Cout, int Cin, int KH, int KW, int64_t so, int64_t si, int64_t sky,
                           int64_t skx, double scale2, void* stream);
/* Style gradient of a modulated conv from the per-sample reductions of its backward (ideas_pixel_dot / ideas_act_bwd_dot), evaluated
 * in DOUBLE (its two terms cancel to a small remainder; stylegan2/model.py:239-248 gets the same gradient from autograd through the
 * materialised per-sample weights):
 *   q[b,o]  = sum_i s[b,i]^2 wsq[o,i],  dt = (q + eps)^(-1/2)                      (re-evaluated here from s and the double wsq)
 *   gq[b,o] = -0.5 * (dot_d[b,o] / d[b,o]) * dt^3      (dL/dq; dot_d = <gy, y>, y = d * conv with d = the f32 factor of the forward)
 *   gs[b,i] = (s != 0 ? dot_s[b,i] / s[b,i] : 0) + 2 s[b,i] * sum_o gq[b,o] * wsq[o,i]      (dot_s = <x, gx>, gx = s * dL/d(s x))
 * d == NULL (no demodulation): only the first term of gs; gq / dot_d / wsq are then unused.
 * dot_d is IN/OUT: on return it holds gq in double (the second launch reads it back; gq is its float copy for ideas_demod_wgrad). */
int ideas_demod_bwd(float* gs, float* gq, const double* dot_s, double* dot_d, const float* d, const float* s, const double* wsq,
                    int B, int Cin, int Cout, float eps, void* stream);
/* Weight gradient through the demodulation, ADDED in place:  gw[o][i][k] += coef * W[o][i][k] * sum_b gq[b,o] * s[b,i]^2
 * (coef = 2 * scale^2).  W has strides (so, si, sky, skx), gw strides (go, gi, gky, gkx). */
int ideas_demod_wgrad(float* gw, const float* w, const float* gq, const float* s, int B, int Cout, int Cin, int KH, int KW, int64_t so,
                      int64_t si, int64_t sky, int64_t skx, int64_t go, int64_t gi, int64_t gky, int64_t gkx, float coef, void* stream);

/* Per-(b,c) sum over pixels of a[b,p,c]*g[b,p,c] (NHWC).  Gives d(style) and d(demod) of the modulated conv
 * without materialising per-sample weights.  out must be ZEROED double[B*C]: products and sums are double throughout (the kernel is
 * HBM-bound; see ideas_demod_bwd for why the width matters).  C <= 6144, B <= 65535 (IDEAS_E_SHAPE above).
 * IDEAS_E_ALIGN: C % 4 == 0 and a or g not 16-byte aligned (the rows are then read four channels at a time); IDEAS_BF16 with
 * C % 4 != 0 (only f32 has the element-wise path; a caller with such bf16 tensors converts them to f32 first).
 * IDEAS_E_UNSUPPORTED: a dtype other than IDEAS_F32 / IDEAS_BF16.  Every check comes before any launch. */
int ideas_pixel_dot(double* out, const void* a, const void* g, int B, int64_t P, int C, int dtype, void* stream);

/* Backward prologue of a fused (modulated conv + bias + leaky-ReLU), NHWC, C % 4 == 0.  One pass over the incoming
 * gradient gy and the saved POST-activation output `out` [B,P,C]:
 *     gpre      = (out > 0 ? gy : gy*alpha) * act_gain
 *     bias_grad[c] += sum_{b,p} gpre                       (ZEROED float[C])
 *     dot[b,c]     += sum_p gpre * (inverse_act(out) - bias[c])   (ZEROED double[B*C]; = <gpre, demodulated conv output>; C <= 3072)
 * so neither the pre-activation tensor nor a separate bias-gradient / pixel-dot pass is needed.
 * gpre_scale (optional float[B*C], 16-byte aligned like bias: both are read four channels at a time): the STORED gpre is
 * multiplied by it (bias_grad and dot are not).  It is meant for the demodulation factor, so that input- and weight-gradient
 * kernels could take the already-scaled gradient; the Python side (op/modulated_conv.py) passes NULL in every precision today and
 * hands the factor to those kernels as their per-sample input scale instead.
 * IDEAS_E_ALIGN: C % 4 != 0, or gpre, gy, out, bias or gpre_scale not 16-byte aligned.  IDEAS_E_SHAPE: C > 3072, B > 65535, a
 * non-positive size.  Every check comes before any launch. */
int ideas_act_bwd_dot(void* gpre, float* bias_grad, double* dot, const void* gy, const void* out, const float* bias,
                      const float* gpre_scale, int B, int64_t P, int C, float alpha, float act_gain, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Minibatch standard deviation of the StyleGAN2 discriminator (stylegan2/model.py:697-705), csrc/minibatch_stddev.hip.
 * x [B,H,W,C] channels-innermost, f32 or bf16 (statistics in f32, chunk sums in double).  G = min(B, group) (<= 16: the group is
 * held in registers), M = B / G, sample n = g*M + m (the group index is the OUTER one), K = (C / feat) * H * W:
 *     mu[m,c,p] = mean_g x[g*M+m,c,p];   u = x - mu;   sd[m,c,p] = sqrt(mean_g u^2 + eps)        (biased, centred first)
 *     s[m,f]    = (1/K) sum_{c in chunk f, p} sd[m,c,p]
 *   ideas_mbstd_fwd   out [B,H,W,C+feat]: out[n,:C] = x[n] (exact), out[n,C+f,p] = s[n % M, f].
 *   ideas_mbstd_bwd   gx [B,H,W,C] = gout[:,:C] + a u / sd with a[m,f] = (sum_{g,p} gout[g*M+m,C+f,p]) / (K G); a_out float[M*feat]
 *                     receives a (the operand of ideas_mbstd_bwd2).
 *   ideas_mbstd_bwd2  the backward of ideas_mbstd_bwd for the cotangent v = ggx [B,H,W,C]:
 *                     dgout [B,H,W,C+feat]: dgout[:,:C] = v, dgout[n,C+f,p] = (1/(K G)) sum_{g, c in chunk f, p} v u / sd;
 *                     dx [B,H,W,C] = a ((v - mean_g v) / sd - u (sum_g v u) / (G sd^3)).
 * workspace (fwd, bwd2): M * feat * IDEAS_MBSTD_MAX_PARTIALS doubles, overwritten (one partial per block; a second small kernel adds
 * them in index order).  No floating-point atomics: the results are bitwise reproducible.  A pixel of out / gout / dgout is C + feat
 * elements, so those tensors are accessed element-wise (no 16-byte alignment is assumed or needed).
 * IDEAS_E_SHAPE: B % G != 0 or C % feat != 0 (the reference's view() raises there too).
 * (Additive within ABI 4: IDEAS_ABI_VERSION stays 4.) */
#define IDEAS_MBSTD_MAX_PARTIALS 64
int ideas_mbstd_fwd(void* out, void* workspace, const void* x, int B, int C, int H, int W, int group, int feat, float eps, int dtype,
                    void* stream);
int ideas_mbstd_bwd(void* gx, float* a_out, const void* gout, const void* x, int B, int C, int H, int W, int group, int feat, float eps,
                    int dtype, void* stream);
int ideas_mbstd_bwd2(void* dgout, void* dx, void* workspace, const void* ggx, const void* x, const float* a_in, int B, int C, int H,
                     int W, int group, int feat, float eps, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Noise injection + bias + leaky-ReLU of a StyledConv (stylegan2/model.py:280-291, 335-341) in one pass, csrc/noise_act.hip.
 * x / out / gy / gx [B,H,W,C] channels-innermost, f32 or bf16 (f32 arithmetic); noise float [noise_batch,H,W] with noise_batch = B
 * or 1 (broadcast over the batch); noise_weight: ONE float in device memory (read by the kernels, never by the host); bias float[C].
 *   ideas_noise_bias_act      out = lrelu(x + noise_weight * noise + bias[c], slope) * scale
 *   ideas_noise_bias_act_bwd  from gy and the saved POST-activation out (sign(out) == sign(pre), as ideas_act_bwd_dot):
 *                             gpre = (out > 0 ? gy : gy * slope) * scale
 *                             gx = gpre;   gbias[c] += sum_{b,p} gpre   (float[C], ADDED to: the caller zeroes it; NULL: skipped)
 *                             gnw[0] = sum_{b,p,c} gpre * noise         (overwritten)
 *                             gnoise[bn,p] = noise_weight * sum_c gpre  (float [noise_batch,H,W], overwritten; summed over b when
 *                                                                        noise_batch = 1; NULL: skipped)
 * 16-byte vectors along C when C % 4 == 0 (% 8 for bf16) and every pointer is 16-byte aligned, an element-wise path for any other C.
 * workspace (bwd): IDEAS_NOISE_ACT_MAX_PARTIALS doubles, followed by B*H*W floats when gnoise is given with noise_batch = 1 < B;
 * overwritten.  gnw is summed without floating-point atomics (one double per block, added in a fixed order by a second small
 * kernel): out, gx, gnw and gnoise are bitwise reproducible.  C <= 8192.
 * IDEAS_E_SHAPE: a non-positive size or a noise_batch other than 1 or B.  (Additive within ABI 4.) */
#define IDEAS_NOISE_ACT_MAX_PARTIALS 2048
int ideas_noise_bias_act(void* out, const void* x, const float* noise, const float* noise_weight, const float* bias, int B, int C,
                         int H, int W, int noise_batch, float slope, float scale, int dtype, void* stream);
int ideas_noise_bias_act_bwd(void* gx, float* gbias, float* gnw, float* gnoise, void* workspace, const void* gy, const void* out,
                             const float* noise, const float* noise_weight, int B, int C, int H, int W, int noise_batch, float slope,
                             float scale, int dtype, void* stream);

/* Adjoint of ReflectionPad2d(pad) in NHWC: gx [B,H,W,C] = fold of gpadded [B,H+2pad,W+2pad,C] (mirrored border rows /
 * columns added back onto their sources), IDEAS_F32 or IDEAS_BF16 (f32 sums, one rounding at the store).  Any C and any
 * element-aligned pointers in both dtypes: 16-byte vectors when C % 4 == 0 (f32) / C % 8 == 0 (bf16) and both pointers are 16-byte
 * aligned, element accesses otherwise; never IDEAS_E_ALIGN.  Used by the input gradient of the reflect-padded 3x3 convs of
 * E / Gstru / Ex (models.py:102-106). */
int ideas_reflect_fold(void* gx, const void* gpadded, int B, int H, int W, int C, int pad, int dtype, void* stream);

/* Fused Adam (beta1 = 0, as every optimiser of train.py:417-432) + optional EMA (utils.py:55-60) over ONE flat f32
 * buffer aliasing all parameters of an optimiser group (n % 4 == 0, 16-byte aligned):
 *     v = beta2*v + (1-beta2)*g*g;  p -= lr * g / (sqrt(v)/sqrt(bias_correction2) + eps);  ema = d*ema + (1-d)*p
 * bias_correction2 = 1 - beta2^step (computed by the caller); ema may be NULL. */
int ideas_adam_ema(float* p, const float* g, float* v, float* ema, int64_t n, float lr, float beta2, float eps,
                   float bias_correction2, float ema_decay, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Input pipeline (dataset.py:10-85 + the transform of train.py:443-449), device side.
 * x_u8: decoded images, uint8 [B][H][W][C] (PIL's HWC order).  y: f32 [B][H][W][C] = the NHWC activation layout.
 *   y = ((x / 255) - mean) / stdv           -- ToTensor then Normalize(mean, stdv), the same two roundings
 * flip_u8 (optional, uint8 [B]): non-zero -> that sample is mirrored horizontally (RandomHorizontalFlip; the caller draws). */
int ideas_image_u8_to_f32(float* y, const void* x_u8, const void* flip_u8, int B, int H, int W, int C, float mean, float stdv,
                          void* stream);

/* ------------------------------------------------------------------------------------------------
 * patchify_image (utils.py:127-149), device side: crop `n_crop` boxes (host int[n_crop][4] = y, x, h, w in source pixels, the
 * same boxes for every image, n_crop <= 64) out of x [B][H][W][C] (NHWC, C = 3 or 1; f32 or bf16) and resize each bilinearly
 * (F.interpolate(mode="bilinear", align_corners=False)) to out_h x out_w.  y: [B * n_crop][out_h][out_w][C], image-major (the
 * torch.stack(patches, 1).view(B * n_crop, ...) order of utils.py:147-149), x's dtype.  One launch for all boxes.
 * ideas_patch_resize_bwd: gx f32 [B][H][W][C] += the adjoint applied to gy (y's shape and dtype); `clear` != 0 zeroes gx first.
 * Overlapping crops accumulate with f32 atomics (the summation order is not fixed, as in torch's own backward).
 * (additive since ABI version 3.) */
int ideas_patch_resize(void* y, const void* x, const int* boxes, int n_crop, int B, int C, int H, int W, int out_h, int out_w,
                       int dtype, void* stream);
int ideas_patch_resize_bwd(float* gx, const void* gy, const int* boxes, int n_crop, int B, int C, int H, int W, int out_h,
                           int out_w, int clear, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The image transforms of adaptive discriminator augmentation (stylegan2/non_leaking.py:316-391), csrc/augment.hip.
 * x / y / gy in `layout` (IDEAS_NCHW or IDEAS_NHWC), f32 or bf16 with f32 arithmetic and one rounding at the store; any C >= 1.
 *   ideas_affine_warp      theta: device float[B][6].  The source position, in pixels of x [B,C,H,W], of output pixel (ox, oy) is
 *                              sx = t0*ox + t1*oy + t2,   sy = t3*ox + t4*oy + t5
 *                          and y[b,c,oy,ox] ([B,C,OH,OW]) is the bilinear blend of the four pixels around (sx, sy); a tap outside
 *                          [0,W-1] x [0,H-1] contributes zero (F.grid_sample(mode="bilinear", padding_mode="zeros"); the host folds
 *                          align_corners=False and the grid's normalisation into theta).  A row of theta that is not finite gives
 *                          zeros for that sample; the tap indices are clamped into the image before any address is formed.
 *   ideas_affine_warp_bwd  the adjoint with respect to x: gx (ALWAYS f32, x's shape and `layout`) += sum over the same taps and
 *                          weights of gy; `clear` != 0 zeroes gx first.  It scatters with f32 atomics, so the order of summation
 *                          is not fixed (as in ideas_patch_resize_bwd and torch's own grid_sample backward).  No gradient for theta.
 *   ideas_color_affine     C = 3.  m: device float[B][12], a row-major 3x4 per sample:
 *                              y[b,i,p] = sum_j m[b][4i+j] * x[b,j,p] + m[b][4i+3]
 *                          Its adjoint is the same call with the transposed 3x3 and a zero last column.
 * NHWC with C % 4 == 0 (f32; C % 8 == 0 for bf16) and 16-byte aligned tensors moves 16-byte vectors along C.
 * IDEAS_E_SHAPE: a non-positive size.  (Additive within ABI 4: IDEAS_ABI_VERSION stays 4.) */
int ideas_affine_warp(void* y, const void* x, const float* theta, int B, int C, int H, int W, int OH, int OW, int layout, int dtype,
                      void* stream);
int ideas_affine_warp_bwd(float* gx, const void* gy, const float* theta, int B, int C, int H, int W, int OH, int OW, int clear,
                          int layout, int dtype, void* stream);
int ideas_color_affine(void* y, const void* x, const float* m, int B, int H, int W, int layout, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LPIPS (VGG): the 2x2 max pool of the backbone and the per-layer head of the learned perceptual distance
 * (stylegan2/lpips/networks_basic.py:64-92, spatial=False, lpips=True), csrc/lpips.hip.
 * Every tensor is [B,H,W,C] channels-innermost, f32 or bf16 with f32 arithmetic and one rounding at the store.
 *   ideas_maxpool2x2_fwd   y [B,H/2,W/2,C] (floor): window 2x2, stride 2, no padding; an odd trailing row / column is in no window.
 *   ideas_maxpool2x2_bwd   gx [B,H,W,C] from gy and the saved input x: gy at the window's maximum, 0 elsewhere, every element of gx
 *                          written exactly once (no memset, no atomics).  Ties go to the first element of the window in row-major
 *                          order; a NaN counts as the maximum (torch's max_pool2d).
 *   ideas_lpips_layer_fwd  f0, f1 [B,H,W,C], w float[C]; d float[B]:
 *                              n_i[p] = sqrt(sum_c f_i[p,c]^2);  u_i = f_i / (n_i + 1e-10)
 *                              d[b]   = (1/(H W)) sum_p sum_c w[c] (u_0[p,c] - u_1[p,c])^2
 *                          workspace: B * IDEAS_LPIPS_MAX_PARTIALS doubles, overwritten (one double per block and sample, added in
 *                          index order by a second small kernel: no floating-point atomics).
 *   ideas_lpips_layer_bwd  gd float[B]; gf0 / gf1 [B,H,W,C], either may be NULL (that gradient is not wanted), not both:
 *                              g_c   = 2 w_c (u_0c - u_1c) gd[b] / (H W)
 *                              gf0_k = g_k / (n_0 + eps) - f0_k (sum_c g_c f0_c) / (n_0 (n_0 + eps)^2);   gf1: the mirror image, negated
 *                          A pixel with n_i = 0 (all features zero) gets gf_i = 0.
 * 16-byte vectors along C when C % 4 == 0 (% 8 for bf16) and every pointer is 16-byte aligned, an element-wise path otherwise.
 * All four are bitwise reproducible.  The head keeps a pixel of both tensors in registers: C <= 2048 (IDEAS_E_UNSUPPORTED above).
 * IDEAS_E_SHAPE: a non-positive size, H < 2 or W < 2 for the pool, B > 65535 for the head.  (Additive within ABI 4.) */
#define IDEAS_LPIPS_MAX_PARTIALS 64
int ideas_maxpool2x2_fwd(void* y, const void* x, int B, int C, int H, int W, int dtype, void* stream);
int ideas_maxpool2x2_bwd(void* gx, const void* gy, const void* x, int B, int C, int H, int W, int dtype, void* stream);
int ideas_lpips_layer_fwd(float* d, void* workspace, const void* f0, const void* f1, const float* w, int B, int C, int H, int W,
                          int dtype, void* stream);
int ideas_lpips_layer_bwd(void* gf0, void* gf1, const float* gd, const void* f0, const void* f1, const float* w, int B, int C, int H,
                          int W, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * FID Inception-v3 (stylegan2/inception.py): the 3x3 pools and the global average of the network, csrc/pool.hip, and the streaming
 * f64 feature statistics of the Frechet distance (stylegan2/fid.py:97-98), csrc/feature_stats.hip.
 *   ideas_pool3x3_fwd      x [B,H,W,C] channels-innermost, f32 or bf16 (f32 arithmetic, one rounding at the store); y by `mode`:
 *       IDEAS_POOL_MAX_S2          F.max_pool2d(x, 3, 2): y [B,(H-3)/2+1,(W-3)/2+1,C], no padding (IDEAS_E_SHAPE for H < 3 or W < 3)
 *       IDEAS_POOL_MAX_S1P1        F.max_pool2d(x, 3, 1, 1): y [B,H,W,C]; a padding tap never wins
 *       IDEAS_POOL_AVG_S1P1_VALID  F.avg_pool2d(x, 3, 1, 1, count_include_pad=False): y [B,H,W,C]; the divisor is the number of
 *                                  in-image taps (4 at corners, 6 at edges, 9 inside); f32 sum in a fixed tap order
 *     In the max modes a NaN counts as the maximum (torch's max_pool2d).  16-byte vectors along C when C % 4 == 0 (% 8 for bf16) and
 *     both pointers are 16-byte aligned, an element-wise path otherwise.
 *   ideas_global_avg_pool  out float [B][C] = the mean over H W of x [B,H,W,C] (adaptive_avg_pool2d(x, 1)), f32 sum in index order.
 *   ideas_feature_stats_accum  x float [N][D]; sum double [D] += sum_n x[n]; gram double [D][D] += x^T x, every product and sum in
 *     f64.  The full matrix is written, symmetric by construction.  Any N >= 1, 1 <= D <= IDEAS_FEATURE_STATS_MAX_DIM
 *     (IDEAS_E_UNSUPPORTED above).  Each element is owned by one thread which adds its N terms in index order to the value already
 *     there: no atomics, and two updates are bitwise one update with the concatenated rows.
 * All three are bitwise reproducible.  IDEAS_E_SHAPE: a non-positive size; IDEAS_E_UNSUPPORTED: a dtype other than f32 / bf16 or
 * an unknown mode; every check comes before any launch.  (Additive within ABI 4: IDEAS_ABI_VERSION stays 4.) */
#define IDEAS_POOL_MAX_S2 0
#define IDEAS_POOL_MAX_S1P1 1
#define IDEAS_POOL_AVG_S1P1_VALID 2
#define IDEAS_FEATURE_STATS_MAX_DIM 4096
int ideas_pool3x3_fwd(void* y, const void* x, int B, int C, int H, int W, int mode, int dtype, void* stream);
int ideas_global_avg_pool(float* out, const void* x, int B, int C, int H, int W, int dtype, void* stream);
int ideas_feature_stats_accum(double* sum, double* gram, const float* x, int N, int D, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Steganography codec (utils.py:74-97 on packed bits) and the container's trip through an 8-bit image file, csrc/stego.hip.
 * Packed bits: one row of nbytes = ceil(L * sigma / 8) bytes per image.  Message bit j of image b is
 *     (row[b][j >> 3] >> (7 - (j & 7))) & 1
 * and element l takes message bits [l * sigma, (l + 1) * sigma), most significant first (the order of message[:, i::sigma]).  The pad
 * bits of the last byte are written as 0 and never counted.  sigma is in 1..8.
 *   ideas_bits_to_tensor   z float [B][L]:  z = step * (num + 0.5) - 1 + ((jitter * r) * 2 - r),  step = 2 / 2^sigma,
 *                          r = (float)(step * delta) (the product in double, rounded once), num = the element's sigma bits as an
 *                          integer, every step one f32 operation in that order: bitwise utils.message_to_tensor.  jitter: U[0,1)
 *                          float [B][L], or NULL: the jitter term is skipped (z is the bin centre).
 *   ideas_tensor_to_bits   z [B][L], f32 or bf16 (widened exactly):  n = (min(max(z, -1), 1) + 1.0f) / step in f32 -- the f32
 *                          rounding of the "+ 1" is part of the reference's decision -- q = min(floor(n), 2^sigma - 1), bit i of the
 *                          element = (q >> (sigma - 1 - i)) & 1: bitwise utils.tensor_to_message.  A NaN decodes as zeros.
 *                          bits (packed rows, may be NULL) receives the decisions; n_err (int [B], may be NULL; needs ref_bits,
 *                          packed rows) receives the number of message bits of image b that differ from ref_bits.  One workgroup per
 *                          image, a fixed-order reduction and one plain store: no atomics, nothing to clear, reproducible.
 *   ideas_image_f32_to_u8  x [B,C,H,W] stored as `layout` (IDEAS_NCHW or IDEAS_NHWC), f32 or bf16, C = 1 or 3.  u8 [B][H][W][C]:
 *                              u8 = trunc(clamp(((clamp(x, -1, 1) + 1) / 2) * 255 + 0.5, 0, 255))
 *                          each step rounded to f32 (utils.image_grid / torchvision's save_image(normalize=True, range=(-1, 1)));
 *                          a NaN gives 0.  y (optional, float [B][H][W][C]) = (u8 / 255 - 0.5) / 0.5, bitwise what
 *                          ideas_image_u8_to_f32 makes of u8: the image a receiver decodes from the file.  NHWC moves four elements
 *                          a lane (16-byte loads and stores of floats) when x, u8 and y are 16-byte aligned, one element otherwise.
 * IDEAS_E_NULL: a required pointer is NULL (z; bits of the encoder; both outputs of the decoder; n_err without ref_bits; u8; x).
 * IDEAS_E_SHAPE: B, L, H or W <= 0, C other than 1 or 3.  IDEAS_E_UNSUPPORTED: sigma outside 1..8, a dtype other than f32 / bf16,
 * an unknown layout.  Every check comes before any launch.  (Additive within ABI 4: IDEAS_ABI_VERSION stays 4.) */
int ideas_bits_to_tensor(float* z, const void* bits, const float* jitter, int B, int L, int sigma, float delta, void* stream);
int ideas_tensor_to_bits(void* bits, int* n_err, const void* z, const void* ref_bits, int B, int L, int sigma, int dtype,
                         void* stream);
int ideas_image_f32_to_u8(void* u8, float* y, const void* x, int B, int C, int H, int W, int layout, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Perceptual path length (stylegan2/ppl.py): the small steps around the generator and the VGG, csrc/ppl.hip and csrc/patchify.hip.
 * B counts PATHS: both tensors of either call hold 2B rows / samples.
 *   ideas_path_endpoints   lat, out float [2B][D] row-major, t float [B].  Rows 2i and 2i + 1 of lat are the ends a, b of path i;
 *                              out[2i] = f(a, b, t[i]),   out[2i + 1] = f(a, b, t[i] + eps)         (the sum formed in f32)
 *                          -- the torch.stack([e0, e1], 1).view(2B, D) order of ppl.py:76.  mode:
 *       IDEAS_PATH_LERP    f = a + (b - a) * t, one rounding per operation in that order (no contraction): bitwise the torch expression
 *       IDEAS_PATH_SLERP   a, b normalised (x / sqrt(sum x^2)); d = a . b; p = t acos(d); c = normalize(b - d a);
 *                          f = normalize(a cos p + c sin p) (ppl.py:16-24).  d is NOT clamped, as in the reference: identical or
 *                          opposite ends (c = 0 / 0) and an all-zero end give a row of NaN there and here.
 *                          One wave per path, both rows from one read of a and b, the row sums as cross-lane butterflies in a fixed
 *                          order (bitwise reproducible, no atomics).  1 <= D <= IDEAS_PATH_MAX_DIM (IDEAS_E_UNSUPPORTED above: a
 *                          path's two rows stay in registers).  16-byte accesses when D % 4 == 0 and lat, out are 16-byte aligned.
 *   ideas_pair_prepare     x [2B][H][W][3], y [2B][out_h][out_w][3], channels-innermost, f32 or bf16 (f32 arithmetic, one rounding
 *                          at the store).  The crop `box` (host int[4] = y, x, h, w in source pixels, inside the image) of every
 *                          sample is resized bilinearly to out_h x out_w (F.interpolate(mode="bilinear", align_corners=False), the
 *                          arithmetic of ideas_patch_resize), then per channel (v - shift[c]) / scale[c] with a true division
 *                          (LPIPS's ScalingLayer; shift, scale: host float[3], copied into the kernel's arguments).  Sample 2i of x
 *                          lands at y[i], sample 2i + 1 at y[B + i]: the two sides of every pair become two contiguous half-batches.
 *                          A box of the output's size has the taps (1, 0): y is (x - shift) / scale bit for bit.  Forward only.
 * IDEAS_E_NULL: a NULL pointer.  IDEAS_E_SHAPE: B, D, H, W, out_h or out_w <= 0, a box that leaves the image or has a non-positive
 * size.  IDEAS_E_UNSUPPORTED: D above the cap, an unknown mode, C != 3, a dtype other than f32 / bf16.  Every check comes before any
 * launch.  (Additive within ABI 4: IDEAS_ABI_VERSION stays 4.) */
#define IDEAS_PATH_LERP 0
#define IDEAS_PATH_SLERP 1
#define IDEAS_PATH_MAX_DIM 4096
int ideas_path_endpoints(float* out, const float* lat, const float* t, float eps, int B, int D, int mode, void* stream);
int ideas_pair_prepare(void* y, const void* x, const int* box, const float* shift, const float* scale, int B, int C, int H, int W,
                       int out_h, int out_w, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Channel attacks on the 8-bit container, csrc/attack.hip: what happens to the bytes ideas_image_f32_to_u8 wrote between sender and
 * receiver.  x_u8 and out_u8 are uint8 [B][H][W][C], C = 1 or 3 (out_u8 must not overlap x_u8).  y (optional, float [B][H][W][C]) =
 * (out_u8 / 255 - 0.5) / 0.5, bitwise what ideas_image_u8_to_f32(mean 0.5, std 0.5) makes of out_u8.
 *
 *   ideas_jpeg_roundtrip   a baseline-JPEG encode and decode at 4:4:4, without the entropy coder (which is lossless), in ONE launch,
 *                          no global scratch buffer, no stores outside out_u8, y and coef.  coef (optional, int16
 *                          [B][C][ceil(H/8)][ceil(W/8)][64]) receives the quantised coefficients of every block at index 8 u + v, u the
 *                          vertical frequency.  The model:
 *     1. Colour, encode side (C = 3), 16-bit fixed point in integers as the IJG library does it:
 *            Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *            Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *            Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
 *        C = 1 has a Y plane only.  (The decimal forms 0.299 ... have exact ties on integer inputs; the result would depend on the
 *        float type.)
 *     2. Padding: H and W are padded up to multiples of 8 by replicating the last row and column (clamped coordinates at load time).
 *     3. Forward DCT: level shift by 128, then the orthonormal 8x8 DCT-II
 *            F(u,v) = 1/4 c(u) c(v) sum_i sum_j f(i,j) cos((2i+1) u pi / 16) cos((2j+1) v pi / 16),   c(0) = 1 / sqrt 2, else 1.
 *     4. Quantiser: the Annex K luminance (Y) and chrominance (Cb, Cr) tables scaled by the IJG quality rule, s = 5000 / quality
 *        (integer division) for quality < 50, else 200 - 2 quality;  T = clamp((base * s + 50) / 100, 1, 255);  quality in 1..100.
 *        Rounding half away from zero:  q = sign(F) floor(|F| / T + 0.5).
 *     5. The four rational coefficients (0,0), (0,4), (4,0), (4,4) are exactly S / 8 with S an integer signed sum of the samples
 *        (signs + - - + + - - + along an axis with frequency 4).  They are quantised in integers: q = sign(S) ((|S| + 4 T) / (8 T)).
 *        Exact ties are common there: every flat block has one.
 *     6. Inverse: q T through the inverse DCT, + 128, floor(v + 0.5), clamp to 0..255.  The four rational coefficients contribute
 *        an integer divided by 8, which enters the sum exactly (their scaling is the constant 1/8, not a product of two rounded
 *        1 / (2 sqrt 2)): a block in which only those four survive comes out bit for bit.
 *     7. Colour, decode side, integers again, each clamped to 0..255:
 *            R = Y + (( 91881 (Cr-128) + 32768) >> 16)
 *            G = Y + ((-22554 (Cb-128) - 46802 (Cr-128) + 32768) >> 16)
 *            B = Y + ((116130 (Cb-128) + 32768) >> 16)
 *        The other 60 coefficients of a block and the samples are f32 sums: they agree with exact arithmetic except within 1.5e-3 of
 *        a rounding tie (in units of F / T and of a grey level; tests/attacks_ref.py derives the figure).
 *     IDEAS_E_NULL: x_u8 or out_u8 is NULL.  IDEAS_E_SHAPE: B, H or W <= 0, C other than 1 or 3.  IDEAS_E_UNSUPPORTED: quality
 *     outside 1..100.  With W % 8 == 0, x_u8 and out_u8 8-byte aligned and y 16-byte aligned a lane moves its 8 pixels as 8-byte
 *     words and float4; any other placement goes byte by byte.
 *
 *   ideas_pixel_attack     intensity, additive Gaussian noise and salt and pepper in one streaming launch.  Each step is rounded to
 *                          f32, no fused multiply-add:
 *            v = ((float)x - 127.5f) * gain + 127.5f + offset              offset in 8-bit levels
 *            v = v + sigma * noise                                          with noise: float [B][H][W][C], standard normal, drawn by
 *                                                                           the caller; sigma in 8-bit levels
 *            r = trunc(clamp(v + 0.5f, 0, 255))                             a NaN gives 0
 *            r = 0 in every channel where u < sp / 2,  255 in every channel where u >= 1 - sp / 2
 *                                                                           with u: float [B][H][W], U[0,1), one draw per pixel
 *     noise may be NULL only with sigma == 0, u only with sp == 0 (IDEAS_E_NULL otherwise, and for x_u8 or out_u8).
 *     IDEAS_E_SHAPE: B, H or W <= 0, C other than 1 or 3.  Four pixels a lane (4-byte words of bytes, float4 of noise, u and y) when
 *     x_u8, out_u8 are 4-byte and noise, u, y 16-byte aligned; one pixel a thread otherwise.
 * Every check comes before any launch.  (Additive within ABI 4: IDEAS_ABI_VERSION stays 4.) */
int ideas_jpeg_roundtrip(void* out_u8, float* y, short* coef, const void* x_u8, int B, int C, int H, int W, int quality, void* stream);
int ideas_pixel_attack(void* out_u8, float* y, const void* x_u8, const float* noise, const float* u, int B, int C, int H, int W,
                       float gain, float offset, float sigma, float sp, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The JPEG file channel, csrc/attack_jpeg.hip: the bytes a decoder reads out of the JPEG FILE that libjpeg 6b / libjpeg-turbo writes
 * with its defaults (what Pillow's Image.save(f, "JPEG", quality=Q) runs): the integer "islow" DCT, 4:2:0 or 4:4:4, fancy upsampling,
 * without the entropy coder (lossless).  Unlike ideas_jpeg_roundtrip above, which is a model in f32 at 4:4:4, all of this is int32 and
 * the result is defined to the byte: tests/jpegfile_ref.py restates it in numpy and tests/test_jpeg_file.py holds that restatement to
 * Pillow's own round trip, byte for byte.  x_u8, out_u8, y as in "Channel attacks".  subsampling: 0 = 4:4:4, 2 = 4:2:0 (Pillow's
 * numbering); checked, but without effect, with C = 1.  coef_y (optional): int16 [B][ceil(H/8)][ceil(W/8)][64].  coef_c (optional, C = 3): int16
 * [B][2][cbh][cbw][64] (Cb, Cr), the chroma block grid being the luma grid at 4:4:4 and ceil(ceil(H/2)/8) x ceil(ceil(W/2)/8) at
 * 4:2:0.  Index 8 u + v, u the vertical frequency.  The model:
 *     1. Colour in: the three fixed-point lines of ideas_jpeg_roundtrip step 1.  C = 1 has one plane.
 *     2. Quantiser tables T: Annex K with the IJG quality rule, as step 4 there (clamp 1..255).
 *     3. Chroma at 4:2:0, ch = ceil(H/2), cw = ceil(W/2).  The full-resolution Cb and Cr planes are padded to an even number of rows
 *        by replicating the last row and to 16 ceil(cw/8) columns by replicating the last column; then
 *            c(i,j) = (p(2i,2j) + p(2i,2j+1) + p(2i+1,2j) + p(2i+1,2j+1) + bias) >> 2,   bias = 1 for even j, 2 for odd j;
 *        then the last row of c is replicated down to 8 ceil(ch/8) rows.  The horizontal padding comes BEFORE the average and the
 *        vertical padding AFTER it: the other orders give other bytes wherever the chroma size is no multiple of 8.
 *     4. Luma, and chroma at 4:4:4: padded to multiples of 8 by replicating the last row and column.
 *     5. Forward DCT per 8x8 block on samples - 128, two passes of the 8-point transform below (rows, then columns), constants
 *        round(c 2^13):  K298 = 2446, K390 = 3196, K541 = 4433, K765 = 6270, K899 = 7373, K1175 = 9633, K1501 = 12299, K1847 = 15137,
 *        K1961 = 16069, K2053 = 16819, K2562 = 20995, K3072 = 25172;  DESCALE(x, n) = (x + (1 << (n-1))) >> n, arithmetic shift.
 *            t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4
 *            t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2,  z = (t12 + t13) K541
 *            rows:    o0 = (t10 + t11) << 2,       o4 = (t10 - t11) << 2,       n = 11
 *            columns: o0 = DESCALE(t10 + t11, 2),  o4 = DESCALE(t10 - t11, 2),  n = 15
 *            o2 = DESCALE(z + t13 K765, n),  o6 = DESCALE(z - t12 K1847, n)
 *            ODD(t4, t5, t6, t7):  z5 = (t4 + t5 + t6 + t7) K1175,  z1 = -(t4 + t7) K899,  z2 = -(t5 + t6) K2562,
 *                                  z3 = z5 - (t4 + t6) K1961,  z4 = z5 - (t5 + t7) K390
 *                                  a4 = t4 K298 + z1 + z3,  a5 = t5 K2053 + z2 + z4,  a6 = t6 K3072 + z2 + z3,  a7 = t7 K1501 + z1 + z4
 *            o7 = DESCALE(a4, n),  o5 = DESCALE(a5, n),  o3 = DESCALE(a6, n),  o1 = DESCALE(a7, n)
 *        The result c is 8 F.
 *     6. Quantiser: q = sign(c) ((|c| + 4 T) / (8 T)), integer division.
 *     7. Inverse on e = q T, columns (n = 11), then rows (n = 18), then + 128 and the clamp to 0..255:
 *            z = (e2 + e6) K541,  t2 = z - e6 K1847,  t3 = z + e2 K765,  t0 = (e0 + e4) << 13,  t1 = (e0 - e4) << 13
 *            t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2,   (a0, a1, a2, a3) = ODD(e7, e5, e3, e1)
 *            o0, o7 = DESCALE(t10 +- a3, n),  o1, o6 = DESCALE(t11 +- a2, n),  o2, o5 = DESCALE(t12 +- a1, n),  o3, o4 = DESCALE(t13 +- a0, n)
 *        (The library's range table wraps outside -512..511 before the + 128; no coefficient set an encoder produces gets there, and
 *        the restatement asserts it.  Every product of both transforms has factors below 2^23 and fits 32 bits; asserted as well.)
 *     8. Chroma up at 4:2:0, on the ch x cw real samples only, neighbour indices clamped to them:
 *            s(i,j) = 3 c(i,j) + c(i',j),   i' = i - 1 for output row 2i, i + 1 for output row 2i + 1
 *            out(., 2j) = (3 s(j) + s(j-1) + 8) >> 4,   out(., 2j+1) = (3 s(j) + s(j+1) + 7) >> 4
 *        Except with cw <= 2 (W <= 4): the library does not filter then, every chroma sample is copied to its 2x2 pixels.
 *     9. Colour out: step 7 of ideas_jpeg_roundtrip.
 * C = 1 and 4:4:4 take one launch and no workspace.  4:2:0 takes two: the first writes the decoded half-resolution Cb and Cr as bytes
 * [B][2][ch][cw] into `workspace` (ideas_jpeg_file_workspace_bytes: 2 B ch cw there, 0 otherwise, and 0 for arguments the round trip
 * refuses), the second reads them with clamped neighbours.  Nothing is written outside out_u8, y, coef_y, coef_c and workspace.  With
 * W % 8 == 0, x_u8 and out_u8 8-byte aligned and y 16-byte aligned a lane moves its 8 pixels as 8-byte words and float4; any other
 * placement goes byte by byte; the same bytes either way.  Speed: not measured on an MI355X (DESIGN.md "Channel attacks").
 * IDEAS_E_NULL: x_u8 or out_u8 is NULL, or workspace is NULL where the size query is non-zero.  IDEAS_E_SHAPE: B, H or W <= 0, C other
 * than 1 or 3.  IDEAS_E_UNSUPPORTED: quality outside 1..100, subsampling other than 0 or 2.  Every check comes before any launch.
 * (Additive within ABI 4: IDEAS_ABI_VERSION stays 4.) */
size_t ideas_jpeg_file_workspace_bytes(int B, int C, int H, int W, int subsampling);
int ideas_jpeg_file_roundtrip(void* out_u8, float* y, short* coef_y, short* coef_c, void* workspace, const void* x_u8, int B, int C,
                              int H, int W, int quality, int subsampling, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The JPEG file, written, csrc/jpeg_bytes.hip: the lossless last step behind ideas_jpeg_file_roundtrip -- from its quantised
 * coefficients coef_y and coef_c to the FILE that libjpeg / libjpeg-turbo writes with its defaults, i.e. the bytes of Pillow's
 * Image.save(f, "JPEG", quality=Q, subsampling=0|2): a baseline file with the standard Huffman tables, not optimised, no restart
 * markers.  Defined to the byte: tests/jpegbytes_ref.py restates it in Python and tests/test_jpeg_bytes.py holds that restatement to
 * Pillow's own files.  The file:
 *   Header (328 bytes for C = 1, 623 for C = 3):
 *     1. FFD8.
 *     2. FFE0 0010 'JFIF\0' 01 01 00 0001 0001 00 00.
 *     3. One DQT segment per table, FFDB 0043 0i and 64 bytes: table i of the quality rule (step 2 of the round trip) in zigzag
 *        order.  i = 0 luma; i = 1 chroma, only with C = 3.
 *     4. FFC0, length 8 + 3 C, 08, H and W as two bytes each, C, then per component id, sampling, table: 1, 22 at 4:2:0 with C = 3
 *        and 11 otherwise, 0;  2, 11, 1;  3, 11, 1.  (C = 1 writes 11 whatever `subsampling` says.  Pillow copies a subsampling of 2
 *        into this one byte of a one-channel file too; the scan, and what a decoder reads, are the same.)
 *     5. One DHT segment per Huffman table in the order DC0 (00), AC0 (10), DC1 (01), AC1 (11), C = 1 the first two only: FFC4,
 *        length 001F (DC) or 00B5 (AC), the id, the 16 counts and the symbols of ISO/IEC 10918-1 Annex K.3 - K.6.
 *     6. FFDA, length 6 + 2 C, C, the pairs (1, 00), (2, 11), (3, 11), then 00 3F 00.
 *   Scan order: MCUs in raster order; an MCU is 8 hs x 8 hs pixels, hs = 2 for C = 3 at 4:2:0 and 1 otherwise; the MCU grid is
 *     ceil(H / 8 hs) x ceil(W / 8 hs), which is also the chroma block grid of coef_c.  Inside an MCU the hs x hs luma blocks in raster
 *     order, then Cb, then Cr.
 *   Dummy luma blocks at 4:2:0: the luma grid of coef_y, ceil(H/8) x ceil(W/8), can be one block short of the MCUs on the right and at
 *     the bottom (wherever ceil(W/8) or ceil(H/8) is odd).  A missing block is coded with all AC zero and the DC of the luma block
 *     before it in the same MCU: a right-edge dummy copies the block on its left; in a dummy bottom row block (1,0) copies (0,1), which
 *     may itself be a dummy, and (1,1) copies (1,0).
 *   Block coding: DC: d = DC - pred, pred the DC of the previous block of the same component in scan order, dummies included, 0 at
 *     the start.  nb = the bit length of |d| (0..11); the code of nb, then the low nb bits of d (d >= 0) or of d - 1 (d < 0).  AC in
 *     zigzag order with r the run of zeros since the last non-zero coefficient: ZRL (F0) while r > 15, then the symbol (r << 4) | nb,
 *     nb = 1..10, and the bits as for DC.  EOB (00) if zeros trail; none when coefficient 63 is non-zero.
 *   End: the last byte is padded with 1 bits; every FF byte of the scan, padding included, is followed by 00; then FFD9.
 *   Size: a block is at most 22 + 63 * 26 = 1660 bits, 208 bytes, twice that stuffed:
 *     ideas_jpeg_file_max_bytes = header + 416 * blocks + 3, blocks counting every block of the scan, dummies included; 0 for
 *     arguments the encoder refuses (C other than 1 or 3, H or W outside 1..65535, subsampling other than 0 or 2, a bound or a
 *     launch beyond 2^31 - 1).
 * files: uint8 [B][row_stride], row_stride >= the bound; nbytes[b] = the length of file b, the bytes behind it unspecified.  An image
 * with a coefficient that has no code (|AC| > 1023, a DC difference beyond +-2047: the entry point takes any int16) gets
 * nbytes[b] = -1 and unspecified bytes inside its row; the other images of the batch are not affected.  workspace:
 * ideas_jpeg_file_encode_workspace_bytes (0 for refused arguments), any alignment, any contents: what needs zeros is cleared on the
 * stream inside the call.  Nothing is written outside files, nbytes and workspace.  Bit and byte offsets inside an image are 64-bit.
 * Four launches behind one memset: one thread a block counts its bits; one workgroup an image turns the counts into offsets; one
 * thread a block writes its bits there (its first and last 32-bit word, shared with the neighbours, by atomicOr: the result does not
 * depend on the order); one workgroup an image writes the header, stuffs and copies the scan and writes FFD9 and the length.  Every grid
 * is exact (no capped grid-stride loop).
 * IDEAS_E_NULL: files, nbytes, coef_y or workspace is NULL, or coef_c with C = 3.  IDEAS_E_SHAPE: B, H or W <= 0, H or W > 65535, C
 * other than 1 or 3, row_stride below the bound, a size the size query answers with 0.  IDEAS_E_UNSUPPORTED: quality outside 1..100,
 * subsampling other than 0 or 2.  Every check comes before any launch.  (Additive within ABI 4: IDEAS_ABI_VERSION stays 4.) */
size_t ideas_jpeg_file_max_bytes(int C, int H, int W, int subsampling);
size_t ideas_jpeg_file_encode_workspace_bytes(int B, int C, int H, int W, int subsampling);
int ideas_jpeg_file_encode(void* files, int* nbytes, long long row_stride, const short* coef_y, const short* coef_c, void* workspace,
                           int B, int C, int H, int W, int quality, int subsampling, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The PNG file, written, csrc/png_bytes.hip: the 8-bit container u8 [B][H][W][C] (C = 1 or 3) as B PNG files that any reader opens to
 * exactly those pixels.  Lossless, and defined to the byte: tests/png_ref.py restates it in numpy and tests/test_png_file.py holds
 * that restatement to zlib's inflate and Pillow's reader.  The deflate stream codes every filtered byte as a Huffman literal: there
 * are NO matches (LZ77), so these are not the bytes zlib would write, and a flat image costs one bit a byte.  The file:
 *   1. The signature 89 'PNG' 0D 0A 1A 0A.
 *   2. IHDR (length 13): W and H as four bytes each (big-endian, as every integer of the framing), bit depth 8, colour type 0 (C = 1)
 *      or 2 (C = 3), compression 0, filter 0, interlace 0.
 *   3. ONE IDAT, then IEND; no other chunk.  Every chunk is length, type, data, CRC-32 of type and data.
 *   4. IDAT's data is a zlib stream: 78 01, the deflate blocks, the Adler-32 of the filtered bytes.
 *   Filtered bytes: per row one type byte 0..4 (None, Sub, Up, Average, Paeth), then the W C residuals (x - prediction) mod 256 with
 *     a the byte C places to the left (bpp = C), b the byte above, c the byte above a; what lies left of the row or above the image is 0.
 *     Average predicts floor((a + b) / 2); Paeth as in the PNG specification: p = a + b - c, the nearest of a, b, c to p, ties in that
 *     order.  b and c are RAW bytes of the row above, so rows do not depend on each other's choice.  The type of a row is the one with
 *     the least sum of |residual|, a residual read as int8 (r < 128 ? r : 256 - r); a tie goes to the lowest type.
 *   Blocks: one deflate block per stripe of IDEAS_PNG_STRIPE_ROWS consecutive rows (the last stripe may be shorter), every block
 *     BTYPE = 2 (dynamic Huffman), BFINAL on the last; the blocks follow each other bit by bit, and the last byte is padded with zeros.
 *     A block is its header, the literal of every filtered byte of the stripe in order, and symbol 256.
 *   The stripe's literal code: over symbols 0..256 with the stripe's byte counts, symbol 256 counted once; at most 15 bits.  Lengths
 *     (the same rule gives the code-length code below, with limit 7):
 *       a. Leaves: the symbols with a non-zero count in ascending (count, symbol).
 *       b. The plain Huffman tree: repeatedly the two lightest nodes become the children of a new internal node; among equal weights a
 *          leaf goes before an internal node, leaves in the order of (a), internal nodes in the order they were made.
 *       c. n[l] = the number of leaves of depth l, depths beyond the limit counted at the limit (and a single leaf at depth 1).
 *       d. While the Kraft sum of n exceeds 1 -- once per 2^-limit it is over: with l the longest length below the limit that has
 *          n[l] > 0: n[l] -= 1, n[l + 1] += 2, n[limit] -= 1 (the step of zlib's gen_bitlen).
 *       e. The lengths are handed out in the order of (a): the first n[limit] leaves get the limit, the next n[limit - 1] one less, ...
 *     Codes: canonical, RFC 1951 3.2.2 (per length counting up in symbol order), packed from the most significant bit of the code as
 *     RFC 1951 3.1.1 asks.  A stripe always has two symbols (a byte and 256), so a stripe of one byte value gets two codes of length 1.
 *   The block header: BFINAL, BTYPE = 2, HLIT = 0 (257 codes: 256 is always in use), HDIST = 0 (ONE distance code, of length 1, never
 *     used: RFC 1951 3.2.7), HCLEN = the least that covers the code-length symbols in use in the order 16 17 18 0 8 7 9 6 10 5 11 4 12
 *     3 13 2 14 1 15 (at least 4), that many 3-bit lengths, then the 257 literal lengths and the distance length 1, each sent as
 *     itself: the run-length symbols 16, 17 and 18 are never used.  The code-length code is built by (a)-(e) from how often each length
 *     0..15 occurs among those 258, with limit 7.  A header is at most 17 + 19 * 3 + 258 * 7 = 1880 bits.
 *   Size: a symbol is at most 15 bits, so with S stripes the stream is at most S * (1880 + 15) + 15 * H * (W C + 1) bits:
 *     ideas_png_file_max_bytes = 43 + ceil(bits / 8) + 20; 0 for arguments the writer refuses (C other than 1 or 3, H or W <= 0, a
 *     bound beyond 2^31 - 1).
 * files: uint8 [B][row_stride], row_stride >= the bound; nbytes[b] = the length of file b, the bytes behind it unspecified (but inside
 * the bound).  workspace: ideas_png_file_encode_workspace_bytes (0 for refused arguments or B * H beyond 2^31 - 1), any alignment, any
 * contents: what needs zeros is cleared on the stream inside the call.  Nothing is written outside files, nbytes and workspace; no
 * host synchronisation, no table copied from the host.  Bit and byte offsets inside an image are 64-bit.
 * Four launches behind one memset: one workgroup a row filters it and adds its bytes to the stripe's histogram; one wave a stripe
 * builds the codes, the header's bits and the stripe's bit count; one workgroup a stripe writes its block at its bit offset (a run's
 * first and last 32-bit word, shared with its neighbours, by atomicOr: the result does not depend on the order); one workgroup an
 * image computes Adler-32 and the CRCs from per-thread slices (a slice's CRC register times x^(8 * bytes behind it) modulo the
 * polynomial), frames the chunks, copies the stream and writes the length.  Every grid is exact.  The result is bitwise reproducible.
 * IDEAS_E_NULL: files, nbytes, u8 or workspace is NULL.  IDEAS_E_SHAPE: B, C, H or W <= 0, row_stride below the bound, a size the size
 * queries answer with 0.  IDEAS_E_UNSUPPORTED: a positive C other than 1 or 3.  Every check comes before any launch.
 * (Additive within ABI 4: IDEAS_ABI_VERSION stays 4.) */
#ifndef IDEAS_PNG_STRIPE_ROWS
#define IDEAS_PNG_STRIPE_ROWS 32
#endif
size_t ideas_png_file_max_bytes(int C, int H, int W);
size_t ideas_png_file_encode_workspace_bytes(int B, int C, int H, int W);
int ideas_png_file_encode(void* files, int* nbytes, long long row_stride, const void* u8, void* workspace, int B, int C, int H, int W,
                          void* stream);

/* ------------------------------------------------------------------------------------------------
 * The JPEG file, read, csrc/jpeg_decode.hip: from the entropy-coded segment of B baseline files to their quantised coefficients and
 * to the pixels libjpeg / libjpeg-turbo decodes -- Pillow's Image.open, to the byte.  tests/jpegdecode_ref.py restates it in Python
 * and tests/test_jpeg_decode.py holds that restatement to Pillow's own pixels.  The header of a file is read on the host
 * (ideas_amd/op/jpeg_decode.py::parse_jpeg), which hands over:
 *   scans: uint8 [B][row_stride].  Row b holds the entropy-coded segment of file b, starting at the first byte after the SOS header and
 *     still stuffed; nbytes[b] bytes of it are valid.  The scan ends at the first FF xx with xx != 00 (normally FFD9), or at nbytes[b]
 *     if there is none (an FF that is the last valid byte is a byte of data).
 *   qt: uint16 [B][C][64], one dequantisation table per image AND per component, in natural order (index 8 u + v, as coef_*), values
 *     1..255: the host resolves the table selectors, and images of different quality can share a call.
 *   huff: [C][2][16 + 256] bytes, for each component its DC and its AC table as the 16 counts and the symbols of a DHT segment, resolved
 *     on the host.  One set per call.
 *   out_u8, y, coef_y (optional), coef_c (optional): as in ideas_jpeg_file_roundtrip, in its layouts.
 *   status[b]: 0 = decoded, -1 = corrupt.
 * C, subsampling, H, W and the MCU, dummy-block and DC-predictor rules are those of "The JPEG file, written" above: a dummy luma block
 * is decoded and dropped, its DC difference counts for the predictor.
 * Corrupt means any of: a bit pattern that is no code of its table; an AC category above 10 or a DC category above 11; a run that
 * passes coefficient 63 (a ZRL counts as a run with a coefficient behind it); a DC outside +-2047 after prediction; the data ending
 * before the last block, i.e. a symbol of a block of the scan that would START at or behind the end of the data; nbytes[b] outside
 * 0..row_stride (the lengths live on the device, so the host cannot refuse them).  An AC symbol 0x10..0xE0 ends the block, as in the
 * library.  A corrupt image's outputs are unspecified but stay inside its rows; the other images of the batch are not affected.
 * Bits after the last block are ignored.  Bits read past the end of the data count as 1.
 * Pixels: steps 7-9 of the file channel with the file's tables, promised to the byte for every file whose coefficients keep the
 * transform inside the bounds tests/jpegfile_ref.py asserts -- every file an encoder made from 8-bit pixels.  Outside them the pixels
 * are unspecified, but the coefficients are still exact and no access leaves a buffer (signed arithmetic wraps: -fwrapv).
 * How: the clean stream is cut into subsequences of IDEAS_JPEG_SUBSEQ_BITS bits.  The decoder's state between two symbols is (bit
 * position, slot of the block in its MCU, zigzag index); one workgroup an image iterates in_i = out_{i-1}, out_i = f_i(in_i) from the
 * guesses in_i = (i L, 0, 0) until nothing changes -- after round r subsequences 0..r are exact, so nsub + 1 rounds are the hard limit
 * and the fixed point does not depend on scheduling; Huffman streams re-synchronise by themselves, so files need few rounds.  Launches
 * behind two to three memsets: unstuff, synchronise, emit (one thread a subsequence: AC values and DC differences), DC prefix sum,
 * pixels (two launches at 4:2:0 with C = 3).  Every grid is exact.  A symbol consumes 1..27 bits, so every inner loop is bounded by
 * the subsequence length + 27 bits whatever the bytes are.
 * workspace: ideas_jpeg_file_decode_workspace_bytes (0 for refused arguments), any alignment, any contents.  An image keeps at most
 * min(row_stride, 208 blocks + 8) clean bytes (what its blocks can need); that many bits must fit 31 bits.  Nothing is written outside
 * out_u8, y, coef_*, status and workspace.
 * IDEAS_E_NULL: out_u8, status, scans, nbytes, qt, huff or workspace is NULL.  IDEAS_E_SHAPE: B, H or W <= 0, H or W > 65535, C other
 * than 1 or 3, row_stride < 1, a size the size query answers with 0.  IDEAS_E_UNSUPPORTED: subsampling other than 0 or 2.  Every
 * check comes before any launch.  (Additive within ABI 4: IDEAS_ABI_VERSION stays 4.) */
#ifndef IDEAS_JPEG_SUBSEQ_BITS          /* (-DIDEAS_JPEG_SUBSEQ_BITS=n: a build for tools/bench_jpeg_decode.py to compare) */
#define IDEAS_JPEG_SUBSEQ_BITS 1024
#endif
size_t ideas_jpeg_file_decode_workspace_bytes(int B, int C, int H, int W, int subsampling, long long row_stride);
int ideas_jpeg_file_decode(void* out_u8, float* y, short* coef_y, short* coef_c, int* status, const void* scans, const int* nbytes,
                           long long row_stride, const unsigned short* qt, const unsigned char* huff, void* workspace, int B, int C,
                           int H, int W, int subsampling, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Spatial channel attacks on the 8-bit container, csrc/attack_spatial.hip: rescaling, Gaussian filtering and median filtering, what
 * a messenger or an image host does to a picture before it re-encodes it.  Integer arithmetic throughout: every result is defined
 * to the byte (tests/spatial_ref.py restates it in numpy; the resize is Pillow's Image.resize(size, Image.BILINEAR) on 8-bit
 * images and the median Pillow's ImageFilter.MedianFilter, byte for byte).  x_u8 is uint8 [B][H][W][C], C = 1 or 3; out_u8 must not
 * overlap it; y (optional, float, the shape of out_u8) = (out_u8 / 255 - 0.5) / 0.5 as in the channel attacks above.
 *
 *   ideas_resample_u8   out_u8 [B][H2][W2][C]: a separable weighted window per output index, given as TABLES (device arrays of
 *                       int32): lo [n_out], the first input index of output i, and kk [n_out][ksize], kk[i][j] the coefficient of
 *                       input lo[i] + j in units of 2^-22, zero-padded to ksize (1 .. IDEAS_RESAMPLE_KMAX).  The model:
 *     1. Horizontal pass, on every input row, with (h_lo, h_kk, h_ksize), n_in = W, n_out = W2:
 *            s = 2^21 + sum_j kk[i][j] * p[clamp(lo[i] + j, 0, n_in - 1)]     in 32-bit integers
 *            byte = clamp(s >> 22, 0, 255)                                     (arithmetic shift of the signed sum)
 *        The result is ROUNDED TO BYTES: the vertical pass sees an 8-bit image [B][H][W2][C].
 *     2. Vertical pass on those bytes with (v_lo, v_kk, v_ksize), n_in = H, n_out = H2, the same two lines.
 *     3. A direction whose two table pointers are both NULL is skipped (its sizes must be equal), as Pillow skips it.
 *     The index is clamped before the load, so a padded tap with coefficient 0 -- or a malformed table -- reads inside the image;
 *     the sum is taken in unsigned 32-bit arithmetic and wraps.  Tables of a proper filter have rows that sum to 2^22 within
 *     ksize / 2 (each coefficient is rounded on its own), so a constant image stays constant.
 *     One launch: a workgroup owns 32 x 64 output pixels, runs the horizontal pass for the input rows its windows reach into LDS
 *     (up to 160 rows of 64 C bytes; 30 KiB at C = 3) and the vertical pass out of LDS.  A tile whose windows reach more rows than
 *     that (none does for a Pillow or Gaussian table within ksize <= 32 and scales 1/4 .. 4; a hand-made table can) computes the
 *     same sums straight from x_u8: the same bytes, no workspace, no second launch.  Four output bytes a thread: one 4-byte store and
 *     one float4 of y when out_u8 is 4-byte aligned, y 16-byte aligned and W2 * C % 4 == 0; byte by byte otherwise.
 *     IDEAS_E_NULL: x_u8 or out_u8 is NULL, or exactly one of a direction's two tables.  IDEAS_E_SHAPE: B, H, W, H2 or W2 <= 0, C
 *     other than 1 or 3, a skipped direction with unequal sizes.  IDEAS_E_UNSUPPORTED: the ksize of a direction that is not skipped
 *     lies outside 1 .. IDEAS_RESAMPLE_KMAX (a skipped direction's ksize is ignored).
 *
 *   ideas_median_u8     out_u8 [B][H][W][C]: per channel the median of the K x K window around each pixel, the image extended by
 *                       replicating its edge rows and columns; K = 3 or 5 (IDEAS_E_UNSUPPORTED otherwise).  One launch: a workgroup
 *                       stages 16 x 64 pixels and their halo in LDS as bytes; a thread finds the medians of four consecutive bytes
 *                       with min/max exchange networks in registers (9 values: the 19-exchange network; 25: forgetful selection,
 *                       132 exchanges).  IDEAS_E_NULL: x_u8 or out_u8 is NULL.  IDEAS_E_SHAPE: B, H or W <= 0, C other than 1 or 3.
 * Every check comes before any launch.  (Additive within ABI 4: IDEAS_ABI_VERSION stays 4.) */
#define IDEAS_RESAMPLE_KMAX 32
int ideas_resample_u8(void* out_u8, void* y, const void* x_u8, int B, int C, int H, int W, int H2, int W2,
                      const int32_t* h_lo, const int32_t* h_kk, int h_ksize,     /* [W2], [W2][h_ksize] */
                      const int32_t* v_lo, const int32_t* v_kk, int v_ksize,     /* [H2], [H2][v_ksize] */
                      void* stream);
int ideas_median_u8(void* out_u8, void* y, const void* x_u8, int B, int C, int H, int W, int K, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Payload coding, csrc/ecc.hip: forward error correction between stego.frame and the secret tensor.  Every image is ONE
 * zero-terminated codeword of a punctured convolutional code, spread over the image's n message bits by an interleaver, and decoded
 * from soft values read off the extractor's output.  The definitions (DESIGN.md "Payload coding"; tests/ecc_ref.py in numpy):
 *   Mother code    r_t = (u_t << 6) | (r_{t-1} >> 1), r_{-1} = 0;  c0 = parity(r_t & 0171), c1 = parity(r_t & 0133) (octal).  The state
 *                  after step t is r_t >> 1: the last six inputs, newest in bit 5.  Input 1,0,0,0,0,0,0 gives 11 10 11 11 00 01 11.
 *   Termination    k information bits (k % 8 == 0) and 6 zero bits: T = k + 6 steps, the path ends in state 0.  T <= 2^20.
 *   Puncturing     periodic in t; rate 1/2: c0 1, c1 1;  2/3: c0 1 1, c1 1 0;  3/4: c0 1 1 0, c1 1 0 1.  The kept outputs are
 *                  numbered i = 0 .. m(T) - 1 in order of t, c0 before c1.  m(T) <= n.
 *   Interleaver    coded position i (0 <= i < n) lives at message bit (i * P) mod n, gcd(P, n) = 1; Pinv is P's inverse mod n.
 *                  Positions i >= m(T) carry fill bits, which the decoder ignores.  Packed rows as in the steganography codec: most significant
 *                  bit first, pad bits of the last byte zero.
 *   Soft value     of message bit j = element l = j / sigma, bit i = j % sigma (most significant first) of z [B][L]:
 *                  c = min(max(z, -1), 1) (a NaN counts as -1); centres c_v = step * (v + 0.5) - 1, step = 2 / 2^sigma;
 *                  d0 / d1 = min (c - c_v)^2 over the v whose bit is 0 / 1;  q = clamp(rint((d0 - d1) / step^2 * gain), -127, 127)
 *                  as int8, positive favours 1.  Every step one f32 operation in that order, no contraction, round-half-even.
 *   Decoder        int32 path metrics, state 0 starts at 0 and the others at -(1 << 30).  The branch metric of a transition is the sum
 *                  over the kept outputs of the step of (c ? +q : -q); it is maximised.  The predecessors of state s' are
 *                  p_b = ((s' & 31) << 1) | b; ON EQUAL METRICS b = 0 WINS (b = 1 only if strictly greater); the survivor bit is b.
 *                  Traceback from state 0; u_t is bit 5 of the state after step t.  No metric normalisation (T <= 2^20).
 *
 *   ideas_ecc_encode   info: packed rows [B][k / 8];  fill: packed rows [B][ceil(n / 8)] or NULL (fill bits 0);  coded: packed rows
 *                      [B][ceil(n / 8)].  A thread owns output bytes and recomputes the parity of the 7-bit window behind each bit.
 *   ideas_ecc_soft     z [B][L] f32 or bf16 (widened exactly) -> soft int8 [B][L * sigma];  gain positive and finite.
 *   ideas_ecc_viterbi  soft int8 [B][n] -> info packed rows [B][k / 8] (whole bytes; nothing else is written) and, if metric is not
 *                      NULL, metric int [B]: the final metric of state 0.  One wave per image, lane = state; the 64 decisions of a
 *                      step are one __ballot word.  The survivors (8 T bytes an image) live in LDS while 8 T <= 32768; a non-NULL
 *                      workspace (uint64 [B][T]) ALWAYS selects the global route, a NULL one above that size is IDEAS_E_UNSUPPORTED.
 *                      Both routes give the same bits.
 * IDEAS_E_NULL: coded, info, soft or z is NULL.  IDEAS_E_SHAPE: B, n, k or L <= 0, k % 8 != 0, k + 6 > 2^20, m(k + 6) > n, P outside
 * [1, n) or gcd(P, n) != 1, P * Pinv mod n != 1.  IDEAS_E_UNSUPPORTED: an unknown rate, sigma outside 1..8, a dtype other than
 * f32 / bf16, a gain that is not positive and finite, survivors above the LDS size without a workspace.  Every check comes before
 * any launch.  (Additive within ABI 4: IDEAS_ABI_VERSION stays 4.) */
#define IDEAS_ECC_RATE_1_2 0
#define IDEAS_ECC_RATE_2_3 1
#define IDEAS_ECC_RATE_3_4 2
int ideas_ecc_encode(void* coded, const void* info, const void* fill, int B, int n, int k, int rate, int P, int Pinv, void* stream);
int ideas_ecc_soft(void* soft, const void* z, int B, int L, int sigma, float gain, int dtype, void* stream);
int ideas_ecc_viterbi(void* info, int* metric, const void* soft, void* workspace, int B, int n, int k, int rate, int P, void* stream);

/* ------------------------------------------------------------------------------------------------
 * EqualLinear (stylegan2/model.py:131-160:  F.linear(input, weight * scale, bias * lr_mul)) for MANY layers sharing one input, one
 * launch per direction.  Replaces the ATen / vendor-GEMM calls behind F.linear on this path: every linear layer of IDEAS is skinny
 * (M = batch <= a few hundred rows, K = 32 .. 8192, N = 1 .. 512), and the generator applies sixteen of them (the modulation layers
 * of its StyledConvs, stylegan2/model.py:226,239) to the same texture code.  (additive since ABI version 3.)
 *
 * A segment = one layer.  All matrices are f32 row-major with explicit row strides (in floats, multiples of 4; 16-byte aligned bases):
 *     w    [n][K]   the layer's weight (ldw)               bias [n] or NULL
 *     y    [M][n]   forward: the output;  backward: the incoming gradient g = dL/dy (ldy)
 *     gw   [n][K]   ideas_linear_bwd_w: the weight gradient (ldgw);   gb [n] or NULL: the bias gradient
 *     scale         the equalised-lr factor (1/sqrt(K) * lr_mul);   bias_mul = lr_mul
 * tile0 / pad_ are scratch of the library (any value).
 *   ideas_linear_fwd     y_s[m][j]   = scale_s * sum_k x[m][k] w_s[j][k] + bias_mul_s * bias_s[j]             (K % 8 == 0)
 *   ideas_linear_bwd_x   gx[m][k]    = sum_s scale_s * sum_j y_s[m][j] w_s[j][k]       (ONE tensor: the sum over the segments, i.e. what
 *                                      autograd would add up for an input used by every layer; n_s % 8 == 0, K % 4 == 0).
 *                                      `workspace`: >= ideas_linear_bwd_x_workspace(sum n_s, M, K) bytes of device scratch
 *                                      (split partial sums, folded in a fixed order: no atomics, reproducible).
 *   ideas_linear_bwd_w   gw_s[j][k] (+)= scale_s * sum_m y_s[m][j] x[m][k];   gb_s[j] (+)= bias_mul_s * sum_m y_s[m][j]
 *                                      (`accumulate` != 0: add to what gw / gb hold -- e.g. the optimiser's gradient buffer; K % 4 == 0)
 * Arithmetic: v_mfma_f32_32x32x2_f32 (exact f32 fused multiply-adds), fixed summation order. */
#define IDEAS_LINEAR_MAX_SEGMENTS 32
typedef struct ideas_linear_seg {
    const float* w;
    const float* bias;
    float* y;
    float* gw;
    float* gb;
    int n, ldw, ldy, ldgw;
    float scale, bias_mul;
    int tile0, pad_;
} ideas_linear_seg;
int ideas_sizeof_linear_seg(void);
int ideas_linear_fwd(const ideas_linear_seg* segs, int nseg, const void* x, int M, int K, int ldx, void* stream);
int64_t ideas_linear_bwd_x_workspace(int total_n, int M, int K);
int ideas_linear_bwd_x(const ideas_linear_seg* segs, int nseg, void* gx, int M, int K, int ldgx, void* workspace,
                       int64_t workspace_bytes, void* stream);
int ideas_linear_bwd_w(const ideas_linear_seg* segs, int nseg, const void* x, int M, int K, int ldx, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IDEAS_HIP_H */
