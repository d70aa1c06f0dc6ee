// upfirdn2d for gfx950: zero-stuff / pad / FIR (flipped) / decimate.
//
// Replaces upfirdn2d_kernel + upfirdn2d_kernel_large (stylegan2/op/upfirdn2d_kernel.cu:49-207).  On the IDEAS path this op is a 4x4
// FIR on channels-last tensors -- the blur (up = down = 1), the decimating FIR in front of a stride-2 skip conv and its adjoint,
// the zero-stuffing FIR -- and pure HBM traffic: read the plane once, write it once.  The kernels:
//   * the 4x4 NHWC schemes, one body each, instantiated over the storage vector (f32 x 4, bf16 x 4, bf16 / f16 x 8) and built from
//     one set of shared pieces: tap staging, factorisation, thread-to-tile decode, fused stage, and a row loader with TWO border
//     policies (clamped + masked loads for the raw 16-byte rows; skipped loads for the 4-channel float windows, load_row_f):
//       blur4_c2           the blur, two output columns per thread, separable window (blur4_bf16x8_c2): the fast path;
//       blur4_f32_c2       the same scheme in its own float4 form (the merged body measured slower in f32, see there)
//       blur4_nhwc         the blur, one column per thread, direct 4x4 window (bf16 at C % 8 == 4)
//       fir4_down2_nhwc    down = 2, direct window, 4 channels per thread
//       fir4_down2_bf16x8  down = 2, separable window, 8 channels per thread
//       fir4_up2           up = 2 (+ residual)
//   * blur_nchw_tile — NCHW (the reference's layout): LDS-staged (TH+kh-1) x (TW+kw-1) input tile per plane.
//   * generic     — any up/down/FIR size, either layout, any dtype, one output per thread (the op's full contract).
#include "common.hpp"

namespace {

struct FirParams {
    int B, C, in_h, in_w, out_h, out_w, kh, kw;
    int up_x, up_y, down_x, down_y, pad_x0, pad_y0;
    float gain;
    int flip;
    int seg_rows;   // the 4x4 NHWC kernels: rows (block rows for up = 2) marched per thread
};

// ---------------- generic: out[oy,ox] = sum_k U[oy*down + ky - pad0] * Kf[ky] ----------------------
// Any up / down / FIR size, either layout, one output per thread.  A = accumulation type and K = the FIR's element type: f32 for
// f32 / bf16 / f16 tensors, f64 for f64.  With `lds_taps` (the host's choice: the table fits GENERIC_TAP_LDS bytes) the flipped,
// gain-scaled taps are staged in LDS; otherwise every tap is formed from the FIR in global memory where it is used (the
// reference's upfirdn2d_kernel_large covers any size as well).  Either way a tap's value is fir[src] * gain, so the two agree.
#define GENERIC_TAP_LDS 32768
template <bool NHWC, typename T, typename A, typename K>
__global__ __launch_bounds__(256) void upfirdn2d_generic(T* __restrict__ y, const T* __restrict__ x,
                                                         const K* __restrict__ fir, FirParams p, int lds_taps) {
    extern __shared__ double s_taps[];
    A* sk = reinterpret_cast<A*>(s_taps);
    if (lds_taps) {
        for (int t = threadIdx.x; t < p.kh * p.kw; t += blockDim.x) {
            int ky = t / p.kw, kx = t % p.kw;
            int src = p.flip ? (p.kh - 1 - ky) * p.kw + (p.kw - 1 - kx) : t;
            sk[t] = (A)fir[src] * (A)p.gain;
        }
        __syncthreads();
    }
    const int64_t total = (int64_t)p.B * p.C * p.out_h * p.out_w;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        int c, ox, oy, b;
        int64_t r = i;
        if (NHWC) {
            c = (int)(r % p.C); r /= p.C;
            ox = (int)(r % p.out_w); r /= p.out_w;
            oy = (int)(r % p.out_h); b = (int)(r / p.out_h);
        } else {
            ox = (int)(r % p.out_w); r /= p.out_w;
            oy = (int)(r % p.out_h); r /= p.out_h;
            c = (int)(r % p.C); b = (int)(r / p.C);
        }
        A acc = 0;
        for (int ky = 0; ky < p.kh; ++ky) {
            int uy = oy * p.down_y + ky - p.pad_y0;
            if (uy < 0 || uy % p.up_y) continue;
            int iy = uy / p.up_y;
            if (iy >= p.in_h) continue;
            for (int kx = 0; kx < p.kw; ++kx) {
                int ux = ox * p.down_x + kx - p.pad_x0;
                if (ux < 0 || ux % p.up_x) continue;
                int ix = ux / p.up_x;
                if (ix >= p.in_w) continue;
                int64_t src = NHWC ? (((int64_t)b * p.in_h + iy) * p.in_w + ix) * p.C + c
                                   : (((int64_t)b * p.C + c) * p.in_h + iy) * p.in_w + ix;
                const A k = lds_taps ? sk[ky * p.kw + kx]
                                     : (A)fir[p.flip ? (p.kh - 1 - ky) * p.kw + (p.kw - 1 - kx) : ky * p.kw + kx] * (A)p.gain;
                acc += ld1(x + src) * k;
            }
        }
        st1(y + i, acc);
    }
}

// ---------------- the 4x4 NHWC kernels: shared pieces ----------------------------------------------------------------------------
// A thread owns one channel vector (4 or 8 channels) of one output column, column pair or 2 x 2 block and marches down a segment of
// rows with its window in registers.  The schemes below differ in the window; taps, decode, loader and fused stage are these.
//
// EPI: a fused elementwise stage on the blurred value before it is stored (ideas_blur_fused):
//   EPI_ACT_BWD   y = (ref > 0 ? v : v * alpha) * scale, bias_grad[c] += sum y    -- blur^T followed by the leaky-ReLU backward
//                                                                                   of the layer below (ref = its saved output)
//   EPI_BIAS_ACT  y = lrelu(v + bias[c], alpha) * scale                           -- the blur of an upsampling conv + FusedLeakyReLU
// Same operation order as bias_act.hip's act_one, so f32 results are bitwise those of blur -> fused_bias_act.
enum { EPI_NONE = 0, EPI_ACT_BWD = 1, EPI_BIAS_ACT = 2 };
struct FirEpi {
    const void* ref;
    const float* bias;
    float* bgrad;
    float alpha, scale;
};
__device__ __forceinline__ float epi_act(float v, float sel, float alpha, float scale) { return (sel > 0.f ? v : v * alpha) * scale; }

// per-thread partial bias gradients -> LDS (one slot per channel) -> one global atomic per channel and block
__device__ __forceinline__ void bgrad_flush(float* s_bg, float* __restrict__ bgrad, int C, bool active, int c0, const float* part, int n) {
    for (int c = threadIdx.x; c < C; c += blockDim.x) s_bg[c] = 0.f;
    __syncthreads();
    if (active)
        for (int e = 0; e < n; ++e) atomicAdd(&s_bg[c0 + e], part[e]);
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const float v = s_bg[c];
        if (v != 0.f) atomicAdd(&bgrad[c], v);
    }
}

// the 16 flipped, gain-scaled taps -> LDS
__device__ __forceinline__ void stage_taps(float (&sk)[16], const float* __restrict__ fir, const FirParams& p) {
    if (threadIdx.x < 16) {
        const int t = threadIdx.x;
        sk[t] = fir[p.flip ? 15 - t : t] * p.gain;
    }
    __syncthreads();
}

// Every FIR of the path is an outer product kv (x) kh (make_kernel, stylegan2/model.py:22-30).  The factorisation is checked on the
// device from the 16 taps: kh = first row, kv = first column / its first element; false (block-uniform) for a rank > 1 table, which
// takes a scheme's direct 16-tap loop.
__device__ __forceinline__ bool factor_taps(const float (&sk)[16], float (&kh)[4], float (&kv)[4]) {
    float kmax = 0.f, res = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) { kh[t] = sk[t]; kv[t] = sk[0] != 0.f ? sk[4 * t] / sk[0] : 0.f; }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) { kmax = fmaxf(kmax, fabsf(sk[4 * j + t])); res = fmaxf(res, fabsf(sk[4 * j + t] - kv[j] * kh[t])); }
    return res <= 1e-6f * kmax;
}

// thread -> (channel vector cv, column col, row segment seg of batch element b: rows r0 .. r1 - 1) on a grid of `cols` columns (or
// column pairs, or 2 x 2 blocks) and `rows` rows; false for the threads past the end.  EPI_ACT_BWD ends in block barriers
// (bgrad_flush), which every lane of every wave has to reach along the SAME path: there the threads past the end redo the last
// thread's work with their stores and their share of the bias gradient masked off, so they are given its tile.
struct Tile { int cv, col, seg, b, r0, r1; };
__device__ __forceinline__ bool decode_tile(Tile& t, const FirParams& p, int CV, int cols, int rows) {
    const int segs = (rows + p.seg_rows - 1) / p.seg_rows;
    const int64_t total = (int64_t)p.B * segs * cols * CV;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < total;
    int64_t r = active ? i : total - 1;
    t.cv = (int)(r % CV); r /= CV;
    t.col = (int)(r % cols); r /= cols;
    t.seg = (int)(r % segs);
    t.b = (int)(r / segs);
    t.r0 = t.seg * p.seg_rows;
    t.r1 = (t.r0 + p.seg_rows < rows) ? t.r0 + p.seg_rows : rows;
    return active;
}

// The three storage vectors as N = 1 << SHIFT floats: f32 x 4 (16 bytes), bf16 x 4 (8 bytes) and eight 2-byte elements E = ideas_bf16
// or _Float16 (16 bytes); arithmetic is f32 for all (exact widening, RNE narrowing, see unpack8 / pack8).
//   mask     the loaded vector, or zeros: component-wise (a ternary on the aggregate becomes a select between ADDRESSES and spills
//            to scratch)
//   round    through the storage type, as a kernel chain that stores the value in between rounds it (the identity for f32)
__device__ __forceinline__ unsigned keep_bits(bool ok) { return ok ? 0xffffffffu : 0u; }
struct VecF32 {
    typedef float4 raw;
    static constexpr int N = 4, SHIFT = 2;
    static __device__ __forceinline__ raw mask(const raw& w, bool ok) { return make_float4(ok ? w.x : 0.f, ok ? w.y : 0.f, ok ? w.z : 0.f, ok ? w.w : 0.f); }
    static __device__ __forceinline__ void unpack(const raw& w, float (&f)[4]) { f[0] = w.x; f[1] = w.y; f[2] = w.z; f[3] = w.w; }
    static __device__ __forceinline__ raw pack(const float (&f)[4]) { return make_float4(f[0], f[1], f[2], f[3]); }
    static __device__ __forceinline__ void round(float (&)[4]) {}
};
struct VecBf16x4 {
    typedef ideas_bf16x4 raw;
    static constexpr int N = 4, SHIFT = 2;
    static __device__ __forceinline__ raw mask(const raw& w, bool ok) {
        const unsigned m = keep_bits(ok);
        raw r;
        r.v = make_uint2(w.v.x & m, w.v.y & m);
        return r;
    }
    static __device__ __forceinline__ void unpack(const raw& w, float (&f)[4]) { VecF32::unpack(to_f4(w), f); }
    static __device__ __forceinline__ raw pack(const float (&f)[4]) { return from_f4<raw>(VecF32::pack(f)); }
    static __device__ __forceinline__ void round(float (&f)[4]) { unpack(pack(f), f); }
};
template <typename E> struct VecX8 {
    typedef uint4 raw;
    static constexpr int N = 8, SHIFT = 3;
    static __device__ __forceinline__ raw mask(const raw& w, bool ok) {
        const unsigned m = keep_bits(ok);
        return make_uint4(w.x & m, w.y & m, w.z & m, w.w & m);
    }
    static __device__ __forceinline__ void unpack(const raw& w, float (&f)[8]) { unpack8(w, f, E{}); }
    static __device__ __forceinline__ raw pack(const float (&f)[8]) { return pack8(f, E{}); }
    static __device__ __forceinline__ void round(float (&f)[8]) { unpack(pack(f), f); }
};
template <int N> struct Fv { float v[N]; };      // one vector's floats, as a value

// r0 k0 + r1 k1 + r2 k2 + r3 k3 as fma(r0, k0, r1 k1) and then one fma per further term.  Written out: left to the compiler's
// contraction, which of the first two products becomes the addend depends on the operand order the vectoriser leaves the sum in, and
// results moved in the last bit with the code around the sum (conv_b3_s2fir.hip restates this order to agree bitwise with the blur).
__device__ __forceinline__ float dot4(float r0, float r1, float r2, float r3, float k0, float k1, float k2, float k3) {
    return fmaf(r3, k3, fmaf(r2, k2, fmaf(r0, k0, r1 * k1)));
}

// bit t: column ix0 + t is inside the image (a bool[NC] ends up in scratch memory)
template <int NC> __device__ __forceinline__ unsigned col_mask(int ix0, int in_w) {
    unsigned m = 0;
#pragma unroll
    for (int t = 0; t < NC; ++t) m |= ((ix0 + t >= 0) && (ix0 + t < in_w)) ? (1u << t) : 0u;
    return m;
}
// columns ix0 .. ix0 + NC - 1 of input row iy (xb: the thread's batch element and channel vector), zeros outside the image.  Loads
// are clamped + masked by value: the address is always a valid one, so NC independent loads are in flight whatever the borders are.
template <typename T, int NC>
__device__ __forceinline__ void load_row(typename T::raw (&dst)[NC], const typename T::raw* __restrict__ xb, int iy, int ix0, unsigned colmask,
                                         const FirParams& p, int CV) {
    const bool rowok = (iy >= 0) && (iy < p.in_h);
    const typename T::raw* xr = xb + (int64_t)(rowok ? iy : 0) * p.in_w * CV;
#pragma unroll
    for (int t = 0; t < NC; ++t) {
        const bool ok = rowok && ((colmask >> t) & 1u);
        dst[t] = T::mask(xr[(int64_t)(ok ? ix0 + t : 0) * CV], ok);
    }
}
// ... as floats.  A second border policy, for the 4-channel windows: they skip the loads outside the image (a branch per vector)
// instead of clamping and masking them -- measured 3-6 % faster there, f32 at 4.4-5.2 TB/s, and the registers they always had.
template <typename T, int NC>
__device__ __forceinline__ void load_row_f(Fv<T::N> (&dst)[NC], const typename T::raw* __restrict__ xb, int iy, int ix0, unsigned colmask,
                                           const FirParams& p, int CV) {
    if constexpr (T::N == 4) {
        const bool rowok = (iy >= 0) && (iy < p.in_h);
        const typename T::raw* xr = xb + ((int64_t)iy * p.in_w + ix0) * CV;
#pragma unroll
        for (int t = 0; t < NC; ++t) {
            dst[t] = Fv<T::N>{};
            if (rowok && ((colmask >> t) & 1u)) T::unpack(xr[(int64_t)t * CV], dst[t].v);
        }
    } else {
        typename T::raw v[NC];
        load_row<T, NC>(v, xb, iy, ix0, colmask, p, CV);
#pragma unroll
        for (int t = 0; t < NC; ++t) T::unpack(v[t], dst[t].v);
    }
}

// the fused stage of one output vector, then its store at yb[off].  The blur is rounded to the storage type first, as the unfused
// blur -> bias_act chain stores it.  rb: ep.ref at yb's position; bb: the thread's biases; bsum: its partial bias gradient.
template <typename T, int EPI>
__device__ __forceinline__ void finish(typename T::raw* __restrict__ yb, const typename T::raw* __restrict__ rb, int64_t off, float (&o)[T::N],
                                       const float (&bb)[T::N], float (&bsum)[T::N], const FirEpi& ep, bool active) {
    if (EPI != EPI_NONE) T::round(o);
    if (EPI == EPI_ACT_BWD) {
        float rf[T::N];
        T::unpack(rb[off], rf);
#pragma unroll
        for (int e = 0; e < T::N; ++e) { o[e] = epi_act(o[e], rf[e], ep.alpha, ep.scale); bsum[e] += o[e]; }
        if (!active) return;
    }
    if (EPI == EPI_BIAS_ACT) {
#pragma unroll
        for (int e = 0; e < T::N; ++e) { const float v = o[e] + bb[e]; o[e] = epi_act(v, v, ep.alpha, ep.scale); }
    }
    yb[off] = T::pack(o);
}

// ---------------- 4x4 blur, up = down = 1, TWO output columns per thread (separable FIR) ------------------------------------------
// A 4x4 window per output issues four loads per output vector and is bound by load instructions, not by HBM (f32: 4.5-5.0 TB/s against
// the 5.5-6 of a plain streaming kernel; bf16 with 8-byte lanes: 1.45 TB/s).  A thread that owns the column pair (2q, 2q+1) loads five
// vectors per row for two outputs (the windows overlap in three columns) and -- the FIR being an outer product, factor_taps -- keeps
// two horizontally filtered values per row instead of a 4 x 5 window: each input row is reduced as it arrives, and the window is
// four of those per column.  A rank > 1 table takes a direct loop.  (Summation order differs from blur4_nhwc in the last bit; fused
// and unfused stages share this body, so they still agree bitwise with each other.)
template <typename T, int EPI>
__device__ __forceinline__ void blur4_c2(typename T::raw* __restrict__ y, const typename T::raw* __restrict__ x, const float* __restrict__ fir,
                                         const FirParams& p, const FirEpi& ep, float (&sk)[16], float* s_bg) {
    typedef typename T::raw raw;
    constexpr int N = T::N;
    stage_taps(sk, fir, p);
    float kh[4], kv[4];
    const bool sep = factor_taps(sk, kh, kv);
    const int CV = p.C >> T::SHIFT;
    Tile tl;
    const bool active = decode_tile(tl, p, CV, (p.out_w + 1) >> 1, p.out_h);
    if (EPI != EPI_ACT_BWD && !active) return;
    const int ox = 2 * tl.col;
    const bool colB = ox + 1 < p.out_w;
    const int oy0 = tl.r0, oy1 = tl.r1;
    const int ix0 = ox - p.pad_x0;
    const raw* xb = x + (int64_t)tl.b * p.in_h * p.in_w * CV + tl.cv;
    raw* yb = y + (((int64_t)tl.b * p.out_h) * p.out_w + ox) * CV + tl.cv;
    const raw* rb = reinterpret_cast<const raw*>(ep.ref) + (((int64_t)tl.b * p.out_h) * p.out_w + ox) * CV + tl.cv;
    float bb[N] = {}, bsum[N] = {};
    if (EPI == EPI_BIAS_ACT) {
#pragma unroll
        for (int e = 0; e < N; ++e) bb[e] = ep.bias[N * tl.cv + e];
    }
    auto fin = [&](int oy, int col, float (&o)[N]) {
        finish<T, EPI>(yb, rb, (int64_t)oy * p.out_w * CV + (int64_t)col * CV, o, bb, bsum, ep, active);
    };
    const unsigned colmask = col_mask<5>(ix0, p.in_w);
    if (!sep) {      // direct 16-tap form, one output at a time: correct for any FIR, not tuned
#pragma unroll 1
        for (int oy = oy0; oy < oy1; ++oy)
#pragma unroll 1
            for (int col = 0; col < (colB ? 2 : 1); ++col) {
                float acc[N] = {};
#pragma unroll 1
                for (int j = 0; j < 4; ++j) {
                    const int iy = oy - p.pad_y0 + j;
                    if (iy < 0 || iy >= p.in_h) continue;
#pragma unroll 1
                    for (int t = 0; t < 4; ++t) {
                        const int ix = ix0 + col + t;
                        if (ix < 0 || ix >= p.in_w) continue;
                        float f[N];
                        T::unpack(xb[((int64_t)iy * p.in_w + ix) * CV], f);
#pragma unroll
                        for (int e = 0; e < N; ++e) acc[e] = fmaf(f[e], sk[4 * j + t], acc[e]);
                    }
                }
                fin(oy, col, acc);
            }
        if (EPI == EPI_ACT_BWD) bgrad_flush(s_bg, ep.bgrad, p.C, active, N * tl.cv, bsum, N);
        return;
    }
    // one input row -> its two horizontally filtered values (columns ox and ox + 1)
    auto hrow = [&](int iy, Fv<N>& ha, Fv<N>& hb) {
        raw v[5];
        load_row<T, 5>(v, xb, iy, ix0, colmask, p, CV);
#pragma unroll
        for (int e = 0; e < N; ++e) { ha.v[e] = 0.f; hb.v[e] = 0.f; }
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            float f[N];
            T::unpack(v[t], f);
#pragma unroll
            for (int e = 0; e < N; ++e) {
                if (t < 4) ha.v[e] = fmaf(f[e], kh[t], ha.v[e]);
                if (t > 0) hb.v[e] = fmaf(f[e], kh[t - 1], hb.v[e]);
            }
        }
    };
    auto emit = [&](int oy, const Fv<N>& a0, const Fv<N>& a1, const Fv<N>& a2, const Fv<N>& a3, const Fv<N>& b0, const Fv<N>& b1, const Fv<N>& b2,
                    const Fv<N>& b3) {
        float o[N];
#pragma unroll
        for (int e = 0; e < N; ++e) o[e] = dot4(a0.v[e], a1.v[e], a2.v[e], a3.v[e], kv[0], kv[1], kv[2], kv[3]);
        fin(oy, 0, o);
        if (colB) {
#pragma unroll
            for (int e = 0; e < N; ++e) o[e] = dot4(b0.v[e], b1.v[e], b2.v[e], b3.v[e], kv[0], kv[1], kv[2], kv[3]);
            fin(oy, 1, o);
        }
    };
    Fv<N> a0, a1, a2, a3, a4, b0, b1, b2, b3, b4;
    {
        const int iy0 = oy0 - p.pad_y0;
        hrow(iy0 + 0, a0, b0); hrow(iy0 + 1, a1, b1); hrow(iy0 + 2, a2, b2);
    }
    int oy = oy0;
#pragma unroll 1
    for (; oy + 1 < oy1; oy += 2) {      // two output rows per trip: ten loads in flight (the window shift is a dependent chain)
        hrow(oy - p.pad_y0 + 3, a3, b3);
        hrow(oy - p.pad_y0 + 4, a4, b4);
        emit(oy, a0, a1, a2, a3, b0, b1, b2, b3);
        emit(oy + 1, a1, a2, a3, a4, b1, b2, b3, b4);
        a0 = a2; a1 = a3; a2 = a4; b0 = b2; b1 = b3; b2 = b4;
    }
    if (oy < oy1) {
        hrow(oy - p.pad_y0 + 3, a3, b3);
        emit(oy, a0, a1, a2, a3, b0, b1, b2, b3);
    }
    if (EPI == EPI_ACT_BWD) bgrad_flush(s_bg, ep.bgrad, p.C, active, N * tl.cv, bsum, N);
}
// (blur4_f32_c2 and blur4_bf16x8_c2: the names bench.py and tools/summarize_profiles.py find these kernels by in a profile)
// The f32 instantiation keeps its own float4 form of that body (the tap, decode and column-mask pieces are the shared ones): as
// blur4_c2<VecF32> the same arithmetic compiled to 82-99 VGPRs against 132 with another load schedule and measured 2-9 % below
// this form on the 128- and 256-pixel shapes, with or without an occupancy hint; this form compiles to the registers and the
// instruction mix it always had (132 / 122 / 98 VGPRs for EPI 0 / 1 / 2).  Its vertical sum r0 kv0 + r1 kv1 + r2 kv2 + r3 kv3 is left to
// the compiler's contraction, which here gives dot4's order (tests/test_fir_pinned_gpu.py holds both forms to the same bytes).
template <int EPI>
__global__ __launch_bounds__(256) void blur4_f32_c2(float4* __restrict__ y, const float4* __restrict__ x,
                                                    const float* __restrict__ fir, FirParams p, FirEpi ep) {
    __shared__ float sk[16];
    extern __shared__ float s_bg[];
    stage_taps(sk, fir, p);
    float kh[4], kv[4];
    const bool sep = factor_taps(sk, kh, kv);
    const int C4 = p.C >> 2;
    Tile tl;
    const bool active = decode_tile(tl, p, C4, (p.out_w + 1) >> 1, p.out_h);
    if (EPI != EPI_ACT_BWD && !active) return;
    const int c4 = tl.cv, b = tl.b, oy0 = tl.r0, oy1 = tl.r1;
    const int ox = 2 * tl.col;
    const bool colB = ox + 1 < p.out_w;
    const int ix0 = ox - p.pad_x0;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 bsum = zero;
    const float4* xb = x + (int64_t)b * p.in_h * p.in_w * C4 + c4;
    float4* yb = y + (((int64_t)b * p.out_h) * p.out_w + ox) * C4 + c4;
    const float4* rb = reinterpret_cast<const float4*>(ep.ref) + (((int64_t)b * p.out_h) * p.out_w + ox) * C4 + c4;
    float4 bb = zero;
    if (EPI == EPI_BIAS_ACT) bb = *reinterpret_cast<const float4*>(ep.bias + 4 * c4);
    auto fin = [&](int oy, int col, float4 acc) {
        const int64_t off = (int64_t)oy * p.out_w * C4 + (int64_t)col * C4;
        if (EPI == EPI_ACT_BWD) {
            const float4 rf = rb[off];
            acc = make_float4(epi_act(acc.x, rf.x, ep.alpha, ep.scale), epi_act(acc.y, rf.y, ep.alpha, ep.scale),
                              epi_act(acc.z, rf.z, ep.alpha, ep.scale), epi_act(acc.w, rf.w, ep.alpha, ep.scale));
            bsum.x += acc.x; bsum.y += acc.y; bsum.z += acc.z; bsum.w += acc.w;
        }
        if (EPI == EPI_ACT_BWD && !active) return;       // (the tail lanes: see decode_tile)
        if (EPI == EPI_BIAS_ACT) {
            const float4 v = make_float4(acc.x + bb.x, acc.y + bb.y, acc.z + bb.z, acc.w + bb.w);
            acc = make_float4(epi_act(v.x, v.x, ep.alpha, ep.scale), epi_act(v.y, v.y, ep.alpha, ep.scale),
                              epi_act(v.z, v.z, ep.alpha, ep.scale), epi_act(v.w, v.w, ep.alpha, ep.scale));
        }
        yb[off] = acc;
    };
    const unsigned colmask = col_mask<5>(ix0, p.in_w);
    if (!sep) {      // direct 16-tap form, one output at a time: correct for any FIR, not tuned
#pragma unroll 1
        for (int oy = oy0; oy < oy1; ++oy)
#pragma unroll 1
            for (int col = 0; col < (colB ? 2 : 1); ++col) {
                float4 acc = zero;
#pragma unroll 1
                for (int j = 0; j < 4; ++j) {
                    const int iy = oy - p.pad_y0 + j;
                    if (iy < 0 || iy >= p.in_h) continue;
#pragma unroll 1
                    for (int t = 0; t < 4; ++t) {
                        const int ix = ix0 + col + t;
                        if (ix < 0 || ix >= p.in_w) continue;
                        const float4 v = xb[((int64_t)iy * p.in_w + ix) * C4];
                        const float kk = sk[4 * j + t];
                        acc.x = fmaf(v.x, kk, acc.x); acc.y = fmaf(v.y, kk, acc.y); acc.z = fmaf(v.z, kk, acc.z); acc.w = fmaf(v.w, kk, acc.w);
                    }
                }
                fin(oy, col, acc);
            }
        if (EPI == EPI_ACT_BWD) {
            const float part[4] = {bsum.x, bsum.y, bsum.z, bsum.w};
            bgrad_flush(s_bg, ep.bgrad, p.C, active, 4 * c4, part, 4);
        }
        return;
    }
    // one input row -> its two horizontally filtered values (columns ox and ox + 1); loads clamped + masked as in load_row
    auto hrow = [&](int iy, float4& ha, float4& hb) {
        const bool rowok = (iy >= 0) && (iy < p.in_h);
        const float4* xr = xb + (int64_t)(rowok ? iy : 0) * p.in_w * C4;
        float4 v[5];
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const bool ok = rowok && ((colmask >> t) & 1u);
            const float4 w = xr[(int64_t)(ok ? ix0 + t : 0) * C4];
            v[t] = make_float4(ok ? w.x : 0.f, ok ? w.y : 0.f, ok ? w.z : 0.f, ok ? w.w : 0.f);
        }
        ha = zero; hb = zero;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            if (t < 4) { ha.x = fmaf(v[t].x, kh[t], ha.x); ha.y = fmaf(v[t].y, kh[t], ha.y); ha.z = fmaf(v[t].z, kh[t], ha.z); ha.w = fmaf(v[t].w, kh[t], ha.w); }
            if (t > 0) { hb.x = fmaf(v[t].x, kh[t - 1], hb.x); hb.y = fmaf(v[t].y, kh[t - 1], hb.y); hb.z = fmaf(v[t].z, kh[t - 1], hb.z); hb.w = fmaf(v[t].w, kh[t - 1], hb.w); }
        }
    };
    auto vsum = [&](const float4& r0, const float4& r1, const float4& r2, const float4& r3) {
        return make_float4(r0.x * kv[0] + r1.x * kv[1] + r2.x * kv[2] + r3.x * kv[3], r0.y * kv[0] + r1.y * kv[1] + r2.y * kv[2] + r3.y * kv[3],
                           r0.z * kv[0] + r1.z * kv[1] + r2.z * kv[2] + r3.z * kv[3], r0.w * kv[0] + r1.w * kv[1] + r2.w * kv[2] + r3.w * kv[3]);
    };
    float4 a0, a1, a2, a3, a4, b0, b1, b2, b3, b4;
    {
        const int iy0 = oy0 - p.pad_y0;
        hrow(iy0 + 0, a0, b0); hrow(iy0 + 1, a1, b1); hrow(iy0 + 2, a2, b2);
    }
    int oy = oy0;
#pragma unroll 1
    for (; oy + 1 < oy1; oy += 2) {      // two output rows per trip: ten 16-byte loads in flight
        hrow(oy - p.pad_y0 + 3, a3, b3);
        hrow(oy - p.pad_y0 + 4, a4, b4);
        fin(oy, 0, vsum(a0, a1, a2, a3));
        if (colB) fin(oy, 1, vsum(b0, b1, b2, b3));
        fin(oy + 1, 0, vsum(a1, a2, a3, a4));
        if (colB) fin(oy + 1, 1, vsum(b1, b2, b3, b4));
        a0 = a2; a1 = a3; a2 = a4; b0 = b2; b1 = b3; b2 = b4;
    }
    if (oy < oy1) {
        hrow(oy - p.pad_y0 + 3, a3, b3);
        fin(oy, 0, vsum(a0, a1, a2, a3));
        if (colB) fin(oy, 1, vsum(b0, b1, b2, b3));
    }
    if (EPI == EPI_ACT_BWD) {
        const float part[4] = {bsum.x, bsum.y, bsum.z, bsum.w};
        bgrad_flush(s_bg, ep.bgrad, p.C, active, 4 * c4, part, 4);
    }
}
template <int EPI, typename E>
__global__ __launch_bounds__(256) void blur4_bf16x8_c2(uint4* __restrict__ y, const uint4* __restrict__ x,
                                                       const float* __restrict__ fir, FirParams p, FirEpi ep) {
    __shared__ float sk[16];
    extern __shared__ float s_bg[];
    blur4_c2<VecX8<E>, EPI>(y, x, fir, p, ep, sk, s_bg);
}

// ---------------- 4x4 blur, up = down = 1, one output column per thread, direct window ---------------------------------------------
// For the channel counts the 8-channel vectors do not divide (bf16, C % 8 == 4): a thread owns 4 channels of one output column and
// marches down the rows with a 4x4 register window w[r][t] (input rows iy0..iy0+3 at columns ix0..ix0+3): four loads and one store
// per output, every access coalesced along C, any FIR.
template <typename T, int EPI>
__global__ __launch_bounds__(256) void blur4_nhwc(typename T::raw* __restrict__ y, const typename T::raw* __restrict__ x,
                                                  const float* __restrict__ fir, FirParams p, FirEpi ep) {
    typedef typename T::raw raw;
    constexpr int N = T::N;
    __shared__ float sk[16];
    extern __shared__ float s_bg[];
    stage_taps(sk, fir, p);
    const int CV = p.C >> T::SHIFT;
    Tile tl;
    const bool active = decode_tile(tl, p, CV, p.out_w, p.out_h);
    if (EPI != EPI_ACT_BWD && !active) return;
    const int ox = tl.col, oy0 = tl.r0, oy1 = tl.r1;
    const int ix0 = ox - p.pad_x0;
    float k[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) k[t] = sk[t];
    const raw* xb = x + (int64_t)tl.b * p.in_h * p.in_w * CV + tl.cv;
    raw* yb = y + (((int64_t)tl.b * p.out_h) * p.out_w + ox) * CV + tl.cv;
    const raw* rb = reinterpret_cast<const raw*>(ep.ref) + (((int64_t)tl.b * p.out_h) * p.out_w + ox) * CV + tl.cv;
    float bb[N] = {}, bsum[N] = {};
    if (EPI == EPI_BIAS_ACT) {
#pragma unroll
        for (int e = 0; e < N; ++e) bb[e] = ep.bias[N * tl.cv + e];
    }
    const unsigned colmask = col_mask<4>(ix0, p.in_w);
    auto row = [&](int iy, Fv<N> (&dst)[4]) { load_row_f<T, 4>(dst, xb, iy, ix0, colmask, p, CV); };
    auto emit = [&](int oy, const Fv<N> (&r0)[4], const Fv<N> (&r1)[4], const Fv<N> (&r2)[4], const Fv<N> (&r3)[4]) {
        float acc[N] = {};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float k0 = k[t], k1 = k[4 + t], k2 = k[8 + t], k3 = k[12 + t];
#pragma unroll
            for (int e = 0; e < N; ++e) acc[e] += r0[t].v[e] * k0 + r1[t].v[e] * k1 + r2[t].v[e] * k2 + r3[t].v[e] * k3;
        }
        finish<T, EPI>(yb, rb, (int64_t)oy * p.out_w * CV, acc, bb, bsum, ep, active);
    };
    Fv<N> w[4][4], w4[4];
    const int iy0 = oy0 - p.pad_y0;
    row(iy0 + 0, w[0]);
    row(iy0 + 1, w[1]);
    row(iy0 + 2, w[2]);
    // two output rows per trip: 8 independent loads in flight instead of 4 (the window shift is a dependent chain, so one row per
    // trip is latency-bound)
    int oy = oy0;
    for (; oy + 1 < oy1; oy += 2) {
        row(oy - p.pad_y0 + 3, w[3]);
        row(oy - p.pad_y0 + 4, w4);
        emit(oy, w[0], w[1], w[2], w[3]);
        emit(oy + 1, w[1], w[2], w[3], w4);
#pragma unroll
        for (int t = 0; t < 4; ++t) { w[0][t] = w[2][t]; w[1][t] = w[3][t]; w[2][t] = w4[t]; }
    }
    if (oy < oy1) {
        row(oy - p.pad_y0 + 3, w[3]);
        emit(oy, w[0], w[1], w[2], w[3]);
    }
    if (EPI == EPI_ACT_BWD) bgrad_flush(s_bg, ep.bgrad, p.C, active, N * tl.cv, bsum, N);
}

// ---------------- 4x4 FIR with decimation by 2 (up = 1, down = 2) ------------------------------------------------------------------
// The blur in front of a 1x1 stride-2 skip conv only feeds every second pixel of every second row into the conv
// (models.py:78-95): computing it at the OUTPUT resolution writes N/4 instead of N and lets the conv run unstrided.
// Two schemes of different arithmetic, both advancing two input rows per output row (8 loads, 1 store per output):
//   fir4_down2_nhwc    4 channels per thread (f32, bf16 at C % 8 == 4): the direct 16-tap window of blur4_nhwc;
//   fir4_down2_bf16x8  8 channels per thread (bf16 / f16 at C % 8 == 0; 8-byte lanes are latency-bound, ~1.5 TB/s): a window of four
//                      horizontally filtered rows (factor_taps; a rank > 1 table takes the direct loop).
template <typename T>
__global__ __launch_bounds__(256) void fir4_down2_nhwc(typename T::raw* __restrict__ y, const typename T::raw* __restrict__ x,
                                                       const float* __restrict__ fir, FirParams p) {
    typedef typename T::raw raw;
    constexpr int N = T::N;
    __shared__ float sk[16];
    stage_taps(sk, fir, p);
    const int CV = p.C >> T::SHIFT;
    Tile tl;
    if (!decode_tile(tl, p, CV, p.out_w, p.out_h)) return;
    const int ix0 = 2 * tl.col - p.pad_x0;
    float k[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) k[t] = sk[t];
    const raw* xb = x + (int64_t)tl.b * p.in_h * p.in_w * CV + tl.cv;
    raw* yb = y + (((int64_t)tl.b * p.out_h) * p.out_w + tl.col) * CV + tl.cv;
    const unsigned colmask = col_mask<4>(ix0, p.in_w);
    Fv<N> w[4][4];
    load_row_f<T, 4>(w[0], xb, 2 * tl.r0 - p.pad_y0 + 0, ix0, colmask, p, CV);
    load_row_f<T, 4>(w[1], xb, 2 * tl.r0 - p.pad_y0 + 1, ix0, colmask, p, CV);
    for (int oy = tl.r0; oy < tl.r1; ++oy) {
        load_row_f<T, 4>(w[2], xb, 2 * oy - p.pad_y0 + 2, ix0, colmask, p, CV);
        load_row_f<T, 4>(w[3], xb, 2 * oy - p.pad_y0 + 3, ix0, colmask, p, CV);
        float acc[N] = {};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int e = 0; e < N; ++e) acc[e] = fmaf(w[j][t].v[e], k[4 * j + t], acc[e]);
        yb[(int64_t)oy * p.out_w * CV] = T::pack(acc);
#pragma unroll
        for (int t = 0; t < 4; ++t) { w[0][t] = w[2][t]; w[1][t] = w[3][t]; }
    }
}

template <typename E>
__global__ __launch_bounds__(256) void fir4_down2_bf16x8(uint4* __restrict__ y, const uint4* __restrict__ x,
                                                         const float* __restrict__ fir, FirParams p) {
    typedef VecX8<E> T;
    constexpr int N = T::N;
    __shared__ float sk[16];
    stage_taps(sk, fir, p);
    float kh[4], kv[4];
    const bool sep = factor_taps(sk, kh, kv);
    const int CV = p.C >> T::SHIFT;
    Tile tl;
    if (!decode_tile(tl, p, CV, p.out_w, p.out_h)) return;
    const int ix0 = 2 * tl.col - p.pad_x0;
    const uint4* xb = x + (int64_t)tl.b * p.in_h * p.in_w * CV + tl.cv;
    uint4* yb = y + (((int64_t)tl.b * p.out_h) * p.out_w + tl.col) * CV + tl.cv;
    const unsigned colmask = col_mask<4>(ix0, p.in_w);
    if (!sep) {      // direct 16-tap form: correct for any FIR, not tuned
#pragma unroll 1
        for (int oy = tl.r0; oy < tl.r1; ++oy) {
            float acc[N] = {};
#pragma unroll 1
            for (int j = 0; j < 4; ++j) {
                Fv<N> row[4];
                load_row_f<T, 4>(row, xb, 2 * oy - p.pad_y0 + j, ix0, colmask, p, CV);
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int e = 0; e < N; ++e) acc[e] = fmaf(row[t].v[e], sk[4 * j + t], acc[e]);
            }
            yb[(int64_t)oy * p.out_w * CV] = T::pack(acc);
        }
        return;
    }
    auto hfilter = [&](const uint4 (&row)[4], Fv<N>& h) {
#pragma unroll
        for (int e = 0; e < N; ++e) h.v[e] = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float f[N];
            T::unpack(row[t], f);
#pragma unroll
            for (int e = 0; e < N; ++e) h.v[e] = fmaf(f[e], kh[t], h.v[e]);
        }
    };
    auto rows2 = [&](int iy, Fv<N>& ha, Fv<N>& hb) {      // input rows iy, iy + 1 -> their horizontally filtered values; 8 loads in flight
        uint4 ra[4], rb[4];
        load_row<T, 4>(ra, xb, iy, ix0, colmask, p, CV);
        load_row<T, 4>(rb, xb, iy + 1, ix0, colmask, p, CV);
        hfilter(ra, ha); hfilter(rb, hb);
    };
    Fv<N> h0, h1, h2, h3;
    rows2(2 * tl.r0 - p.pad_y0, h0, h1);
#pragma unroll 1
    for (int oy = tl.r0; oy < tl.r1; ++oy) {
        rows2(2 * oy - p.pad_y0 + 2, h2, h3);
        float o[N];
#pragma unroll
        for (int e = 0; e < N; ++e) o[e] = dot4(h0.v[e], h1.v[e], h2.v[e], h3.v[e], kv[0], kv[1], kv[2], kv[3]);
        yb[(int64_t)oy * p.out_w * CV] = T::pack(o);
        h0 = h2; h1 = h3;
    }
}

// ---------------- 4x4 FIR after zero-stuffing by 2 (up = 2, down = 1) ---------------------------------------------------------------
// The adjoint of the kernels above (their backward), and the blur behind a 1x1 stride-2 TRANSPOSED skip conv (three of four
// pixels of that conv's output are structural zeros; here they are never written or read).  Per axis, output o = 2i + a
// (a = 0, 1) sees the two taps k = k0(a), k0(a) + 2 with k0(a) = (pad0 - a) & 1, at inputs i + d(a), i + d(a) + 1,
// d(a) = (a + k0(a) - pad0) / 2 -- so a 2 x 2 output block needs a 3 x 3 input neighbourhood, kept in registers (72 floats at 8
// channels).  A thread owns the output column pair (2j, 2j + 1) of one channel vector and marches down block rows: 3 loads and 4
// stores per block row.  Never assumes separability.
// `resid` (optional, same shape as y): y = fir(x) + resid -- the residual merge behind an upsampling skip, and (as the adjoint of
// fir4_down2) the sum of the two input gradients of a downsampling ResBlock, without a separate add pass (ideas_fir_up2_add).
template <typename T>
__global__ __launch_bounds__(256) void fir4_up2(typename T::raw* __restrict__ y, const typename T::raw* __restrict__ x,
                                                const float* __restrict__ fir, FirParams p, const typename T::raw* __restrict__ resid) {
    typedef typename T::raw raw;
    constexpr int N = T::N;
    __shared__ float sk[16];
    stage_taps(sk, fir, p);
    const int CV = p.C >> T::SHIFT;
    const int bh = (p.out_h + 1) >> 1, bw = (p.out_w + 1) >> 1;          // 2 x 2 output blocks
    Tile tl;
    if (!decode_tile(tl, p, CV, bw, bh)) return;
    const int j = tl.col;
    // per-axis tap / offset tables (a = output parity)
    const int ky0[2] = {p.pad_y0 & 1, (p.pad_y0 - 1) & 1}, kx0[2] = {p.pad_x0 & 1, (p.pad_x0 - 1) & 1};
    const int dy[2] = {(ky0[0] - p.pad_y0) >> 1, (1 + ky0[1] - p.pad_y0) >> 1};
    const int dx[2] = {(kx0[0] - p.pad_x0) >> 1, (1 + kx0[1] - p.pad_x0) >> 1};
    const int ey = dy[1] - dy[0], ex = dx[1] - dx[0];                       // 0 or 1: which 2 of the 3 rows / columns parity 1 uses
    float wq[2][2][2][2];                                                  // [a][bb][u][v]
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int bb = 0; bb < 2; ++bb)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int v = 0; v < 2; ++v) wq[a][bb][u][v] = sk[(ky0[a] + 2 * u) * 4 + kx0[bb] + 2 * v];
    const raw* xb = x + (int64_t)tl.b * p.in_h * p.in_w * CV + tl.cv;
    const int cx0 = j + dx[0];
    const unsigned colmask = col_mask<3>(cx0, p.in_w);
    Fv<N> R0[3], R1[3], R2[3];
    load_row_f<T, 3>(R0, xb, tl.r0 + dy[0] + 0, cx0, colmask, p, CV);
    load_row_f<T, 3>(R1, xb, tl.r0 + dy[0] + 1, cx0, colmask, p, CV);
    const bool colB = 2 * j + 1 < p.out_w;
#pragma unroll 1
    for (int i = tl.r0; i < tl.r1; ++i) {
        load_row_f<T, 3>(R2, xb, i + dy[0] + 2, cx0, colmask, p, CV);
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int oy = 2 * i + a;
            if (oy >= p.out_h) break;
            const bool hi = (a == 1) && (ey == 1);      // rows of this parity: R[ra], R[ra + 1] with ra = a ? ey : 0 (no dynamic register indexing)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) {
                if (bb == 1 && !colB) break;
                const bool hx = (bb == 1) && (ex == 1);
                const float w00 = wq[a][bb][0][0], w01 = wq[a][bb][0][1], w10 = wq[a][bb][1][0], w11 = wq[a][bb][1][1];
                float o[N];
#pragma unroll
                for (int e = 0; e < N; ++e) {
                    const float top0 = hi ? R1[0].v[e] : R0[0].v[e], top1 = hi ? R1[1].v[e] : R0[1].v[e], top2 = hi ? R1[2].v[e] : R0[2].v[e];
                    const float bot0 = hi ? R2[0].v[e] : R1[0].v[e], bot1 = hi ? R2[1].v[e] : R1[1].v[e], bot2 = hi ? R2[2].v[e] : R1[2].v[e];
                    const float t0 = hx ? top1 : top0, t1 = hx ? top2 : top1, b0 = hx ? bot1 : bot0, b1 = hx ? bot2 : bot1;
                    o[e] = dot4(t0, t1, b0, b1, w00, w01, w10, w11);
                }
                const int64_t yi = (((int64_t)tl.b * p.out_h + oy) * p.out_w + 2 * j + bb) * CV + tl.cv;
                if (resid) {
                    T::round(o);          // the two-kernel chain stores the FIR first
                    float rf[N];
                    T::unpack(resid[yi], rf);
#pragma unroll
                    for (int e = 0; e < N; ++e) o[e] += rf[e];
                }
                y[yi] = T::pack(o);
            }
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) { R0[t] = R1[t]; R1[t] = R2[t]; }
    }
}

// ---------------- NCHW tiled blur, up = down = 1, k <= 4 -------------------------------------------
#define TNH 16
#define TNW 64
// T = float or _Float16 (the reference's half layout); the tile and the arithmetic are f32 for both
template <typename T>
__global__ __launch_bounds__(256) void blur_nchw_tile(T* __restrict__ y, const T* __restrict__ x,
                                                      const float* __restrict__ fir, FirParams p) {
    __shared__ float sk[16];
    __shared__ float sx[TNH + 3][TNW + 3 + 1];
    if (threadIdx.x < 16) {
        int t = threadIdx.x;
        int ky = t >> 2, kx = t & 3;
        float v = 0.f;
        if (ky < p.kh && kx < p.kw) {
            int src = p.flip ? (p.kh - 1 - ky) * p.kw + (p.kw - 1 - kx) : ky * p.kw + kx;
            v = fir[src] * p.gain;
        }
        sk[t] = v;
    }
    const int tiles_x = (p.out_w + TNW - 1) / TNW;
    const int tiles_y = (p.out_h + TNH - 1) / TNH;
    int64_t bid = blockIdx.x;
    const int tx = (int)(bid % tiles_x); bid /= tiles_x;
    const int ty = (int)(bid % tiles_y);
    const int64_t plane = bid / tiles_y;
    const int oy0 = ty * TNH, ox0 = tx * TNW;
    const T* xp = x + plane * p.in_h * p.in_w;
    for (int t = threadIdx.x; t < (TNH + 3) * (TNW + 3); t += blockDim.x) {
        int ry = t / (TNW + 3), rx = t % (TNW + 3);
        int iy = oy0 + ry - p.pad_y0, ix = ox0 + rx - p.pad_x0;
        float v = 0.f;
        if (iy >= 0 && iy < p.in_h && ix >= 0 && ix < p.in_w) v = ld1(xp + (int64_t)iy * p.in_w + ix);
        sx[ry][rx] = v;
    }
    __syncthreads();
    T* yp = y + plane * p.out_h * p.out_w;
    for (int t = threadIdx.x; t < TNH * TNW; t += blockDim.x) {
        int ry = t / TNW, rx = t % TNW;
        int oy = oy0 + ry, ox = ox0 + rx;
        if (oy >= p.out_h || ox >= p.out_w) continue;
        float acc = 0.f;
#pragma unroll
        for (int ky = 0; ky < 4; ++ky)
#pragma unroll
            for (int kx = 0; kx < 4; ++kx) acc += sx[ry + ky][rx + kx] * sk[ky * 4 + kx];
        st1(yp + (int64_t)oy * p.out_w + ox, acc);
    }
}

}  // namespace

// one thread per tile: 256-thread blocks over `total` threads
#define FIR_LAUNCH(kernel, total, lds, stream, ...) \
    hipLaunchKernelGGL(kernel, dim3((unsigned)ideas_cdiv((int64_t)(total), 256)), dim3(256), lds, stream, __VA_ARGS__)

// the unit-stride 4x4 NHWC blur (+ fused stage): shared by ideas_upfirdn2d (EPI_NONE) and ideas_blur_fused
template <int EPI>
static int launch_blur4(void* y, const void* x, const float* fir, FirParams p, FirEpi ep, int dtype, hipStream_t stream) {
    // rows marched per thread: each segment re-reads 3 halo rows (19/16 of the input).  With the two-column kernels (half the
    // threads per row) 16 beats 8 / 24 / 32 / 64 at every size: 5.3-5.5 TB/s against 4.9-5.0 (32) in f32 at 256x256
    p.seg_rows = 16;
    const int segs = (p.out_h + p.seg_rows - 1) / p.seg_rows;
    const int64_t total = (int64_t)p.B * segs * p.out_w * (p.C / 4);
    if (ideas_cdiv(total, 256) > 0x7fffffffLL) return IDEAS_E_SHAPE;
    const size_t lds = EPI == EPI_ACT_BWD ? (size_t)p.C * sizeof(float) : 0;
    const int64_t pairs = (int64_t)p.B * segs * ((p.out_w + 1) / 2);          // column pairs: the two-column kernels
    if constexpr (EPI == EPI_NONE) {          // f16 (C % 8 == 0, plain blur only): the 8-channel two-column kernel of bf16
        if (dtype == IDEAS_F16) {
            FIR_LAUNCH((blur4_bf16x8_c2<EPI, _Float16>), pairs * (p.C / 8), lds, stream, (uint4*)y, (const uint4*)x, fir, p, ep);
            return ideas_launch_status();
        }
    }
    if (dtype == IDEAS_BF16 && p.C % 8 == 0)
        FIR_LAUNCH((blur4_bf16x8_c2<EPI, ideas_bf16>), pairs * (p.C / 8), lds, stream, (uint4*)y, (const uint4*)x, fir, p, ep);
    else if (dtype == IDEAS_BF16)
        FIR_LAUNCH((blur4_nhwc<VecBf16x4, EPI>), total, lds, stream, (ideas_bf16x4*)y, (const ideas_bf16x4*)x, fir, p, ep);
    else
        FIR_LAUNCH(blur4_f32_c2<EPI>, pairs * (p.C / 4), lds, stream, (float4*)y, (const float4*)x, fir, p, ep);
    return ideas_launch_status();
}

// down = 2 / up = 2: `tiles` = batch x row segments x columns (column pairs for up = 2); x8: 8 channels per thread (bf16 / f16)
static void launch_down2(void* y, const void* x, const float* fir, const FirParams& p, int64_t tiles, int dtype, bool x8, hipStream_t stream) {
    if (x8 && dtype == IDEAS_F16)
        FIR_LAUNCH(fir4_down2_bf16x8<_Float16>, tiles * (p.C / 8), 0, stream, (uint4*)y, (const uint4*)x, fir, p);
    else if (x8)
        FIR_LAUNCH(fir4_down2_bf16x8<ideas_bf16>, tiles * (p.C / 8), 0, stream, (uint4*)y, (const uint4*)x, fir, p);
    else if (dtype == IDEAS_BF16)
        FIR_LAUNCH(fir4_down2_nhwc<VecBf16x4>, tiles * (p.C / 4), 0, stream, (ideas_bf16x4*)y, (const ideas_bf16x4*)x, fir, p);
    else
        FIR_LAUNCH(fir4_down2_nhwc<VecF32>, tiles * (p.C / 4), 0, stream, (float4*)y, (const float4*)x, fir, p);
}
static void launch_up2(void* y, const void* x, const float* fir, const FirParams& p, const void* resid, int64_t tiles, int dtype, bool x8,
                       hipStream_t stream) {
    if (x8 && dtype == IDEAS_F16)
        FIR_LAUNCH(fir4_up2<VecX8<_Float16>>, tiles * (p.C / 8), 0, stream, (uint4*)y, (const uint4*)x, fir, p, (const uint4*)resid);
    else if (x8)
        FIR_LAUNCH(fir4_up2<VecX8<ideas_bf16>>, tiles * (p.C / 8), 0, stream, (uint4*)y, (const uint4*)x, fir, p, (const uint4*)resid);
    else if (dtype == IDEAS_BF16)
        FIR_LAUNCH(fir4_up2<VecBf16x4>, tiles * (p.C / 4), 0, stream, (ideas_bf16x4*)y, (const ideas_bf16x4*)x, fir, p, (const ideas_bf16x4*)resid);
    else
        FIR_LAUNCH(fir4_up2<VecF32>, tiles * (p.C / 4), 0, stream, (float4*)y, (const float4*)x, fir, p, (const float4*)resid);
}

#undef FIR_LAUNCH

extern "C" int ideas_blur_fused(void* y, const void* x, const float* fir, int B, int C, int in_h, int in_w, int out_h, int out_w,
                                int pad_x0, int pad_y0, float gain, int flip, int mode, const void* ref, const float* bias,
                                float* bias_grad, float alpha, float scale, int dtype, void* stream_) {
    if (dtype != IDEAS_F32 && dtype != IDEAS_BF16) return IDEAS_E_UNSUPPORTED;
    if (!y || !x || !fir) return IDEAS_E_NULL;
    if (B <= 0 || C <= 0 || in_h <= 0 || in_w <= 0 || out_h <= 0 || out_w <= 0) return IDEAS_E_SHAPE;
    if (C % 4 || C > 8192) return IDEAS_E_UNSUPPORTED;
    if (!ideas_aligned16(x) || !ideas_aligned16(y)) return IDEAS_E_ALIGN;
    FirParams p{B, C, in_h, in_w, out_h, out_w, 4, 4, 1, 1, 1, 1, pad_x0, pad_y0, gain, flip, 16};
    FirEpi ep{ref, bias, bias_grad, alpha, scale};
    hipStream_t stream = (hipStream_t)stream_;
    if (mode == EPI_ACT_BWD) {
        if (!ref || !bias_grad) return IDEAS_E_NULL;
        if (!ideas_aligned16(ref)) return IDEAS_E_ALIGN;
        return launch_blur4<EPI_ACT_BWD>(y, x, fir, p, ep, dtype, stream);
    }
    if (mode == EPI_BIAS_ACT) {
        if (!bias) return IDEAS_E_NULL;
        if (!ideas_aligned16(bias)) return IDEAS_E_ALIGN;
        return launch_blur4<EPI_BIAS_ACT>(y, x, fir, p, ep, dtype, stream);
    }
    return IDEAS_E_UNSUPPORTED;
}

static int upfirdn2d_impl(void* y, const void* x, const float* fir, int B, int C, int in_h, int in_w, int out_h,
                          int out_w, int kh, int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0,
                          int pad_y0, float gain, int flip, int layout, int dtype, void* stream_, const void* resid) {
    if (dtype != IDEAS_F32 && dtype != IDEAS_BF16 && dtype != IDEAS_F16 && dtype != IDEAS_F64) return IDEAS_E_UNSUPPORTED;
    if (dtype == IDEAS_BF16 && layout != IDEAS_NHWC) return IDEAS_E_UNSUPPORTED;
    if (!y || !x || !fir) return IDEAS_E_NULL;
    if (B <= 0 || C <= 0 || in_h <= 0 || in_w <= 0 || out_h <= 0 || out_w <= 0) return IDEAS_E_SHAPE;
    if (kh <= 0 || kw <= 0) return IDEAS_E_UNSUPPORTED;
    if (up_x <= 0 || up_y <= 0 || down_x <= 0 || down_y <= 0) return IDEAS_E_SHAPE;
    if (layout != IDEAS_NCHW && layout != IDEAS_NHWC) return IDEAS_E_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    FirParams p{B, C, in_h, in_w, out_h, out_w, kh, kw, up_x, up_y, down_x, down_y, pad_x0, pad_y0, gain, flip, 16};
    const bool unit = up_x == 1 && up_y == 1 && down_x == 1 && down_y == 1;
    // the 4x4 NHWC kernels: f32 / bf16 at C % 4 == 0, f16 at C % 8 == 0 (8 channels per thread only); f64 has none
    const bool fast = dtype == IDEAS_F32 || dtype == IDEAS_BF16 || (dtype == IDEAS_F16 && C % 8 == 0);
    const bool vec4 = fast && layout == IDEAS_NHWC && kh == 4 && kw == 4 && (C % 4 == 0) && ideas_aligned16(x) && ideas_aligned16(y);
    const bool x8 = (dtype == IDEAS_BF16 || dtype == IDEAS_F16) && C % 8 == 0;
    if (unit && vec4) {
        return launch_blur4<EPI_NONE>(y, x, fir, p, FirEpi{nullptr, nullptr, nullptr, 0.f, 1.f}, dtype, stream);
    }
    if (vec4 && up_x == 1 && up_y == 1 && down_x == 2 && down_y == 2) {
        p.seg_rows = out_h >= 64 ? 16 : 8;
        const int segs = (out_h + p.seg_rows - 1) / p.seg_rows;
        const int64_t tiles = (int64_t)B * segs * out_w;
        if (ideas_cdiv(tiles * (C / 4), 256) > 0x7fffffffLL) return IDEAS_E_SHAPE;
        launch_down2(y, x, fir, p, tiles, dtype, x8, stream);
        return ideas_launch_status();
    }
    if (resid && !(vec4 && up_x == 2 && up_y == 2 && down_x == 1 && down_y == 1 && ideas_aligned16(resid))) return IDEAS_E_UNSUPPORTED;
    if (vec4 && up_x == 2 && up_y == 2 && down_x == 1 && down_y == 1) {
        const int bh = (out_h + 1) / 2, bw = (out_w + 1) / 2;
        p.seg_rows = bh >= 64 ? 16 : 8;
        const int segs = (bh + p.seg_rows - 1) / p.seg_rows;
        const int64_t tiles = (int64_t)B * segs * bw;
        if (ideas_cdiv(tiles * (C / 4), 256) > 0x7fffffffLL) return IDEAS_E_SHAPE;
        launch_up2(y, x, fir, p, resid, tiles, dtype, x8, stream);
        return ideas_launch_status();
    }
    if (unit && layout == IDEAS_NCHW && kh <= 4 && kw <= 4 && (dtype == IDEAS_F32 || dtype == IDEAS_F16)) {
        const int64_t grid = (int64_t)B * C * ideas_cdiv(out_h, TNH) * ideas_cdiv(out_w, TNW);
        if (grid > 0x7fffffffLL) return IDEAS_E_SHAPE;
        if (dtype == IDEAS_F16)
            hipLaunchKernelGGL(blur_nchw_tile<_Float16>, dim3((unsigned)grid), dim3(256), 0, stream, (_Float16*)y, (const _Float16*)x, fir, p);
        else
            hipLaunchKernelGGL(blur_nchw_tile<float>, dim3((unsigned)grid), dim3(256), 0, stream, (float*)y, (const float*)x, fir, p);
        return ideas_launch_status();
    }
    const int64_t total = (int64_t)B * C * out_h * out_w;
    int64_t grid = ideas_cdiv(total, 256);
    if (grid > 65536) grid = 65536;
    const int64_t tap_bytes = (int64_t)kh * kw * (dtype == IDEAS_F64 ? sizeof(double) : sizeof(float));
    const int lds_taps = tap_bytes <= GENERIC_TAP_LDS;
    const size_t lds = lds_taps ? (size_t)tap_bytes : 0;
    const dim3 g((unsigned)grid), blk(256);
    const bool nhwc = layout == IDEAS_NHWC;
    if (dtype == IDEAS_BF16)
        hipLaunchKernelGGL((upfirdn2d_generic<true, ideas_bf16, float, float>), g, blk, lds, stream, (ideas_bf16*)y,
                           (const ideas_bf16*)x, fir, p, lds_taps);
    else if (dtype == IDEAS_F16 && nhwc)
        hipLaunchKernelGGL((upfirdn2d_generic<true, _Float16, float, float>), g, blk, lds, stream, (_Float16*)y, (const _Float16*)x,
                           fir, p, lds_taps);
    else if (dtype == IDEAS_F16)
        hipLaunchKernelGGL((upfirdn2d_generic<false, _Float16, float, float>), g, blk, lds, stream, (_Float16*)y, (const _Float16*)x,
                           fir, p, lds_taps);
    else if (dtype == IDEAS_F64 && nhwc)          // f64: `fir` points to double (include/ideas_hip.h)
        hipLaunchKernelGGL((upfirdn2d_generic<true, double, double, double>), g, blk, lds, stream, (double*)y, (const double*)x,
                           (const double*)fir, p, lds_taps);
    else if (dtype == IDEAS_F64)
        hipLaunchKernelGGL((upfirdn2d_generic<false, double, double, double>), g, blk, lds, stream, (double*)y, (const double*)x,
                           (const double*)fir, p, lds_taps);
    else if (nhwc)
        hipLaunchKernelGGL((upfirdn2d_generic<true, float, float, float>), g, blk, lds, stream, (float*)y, (const float*)x, fir, p,
                           lds_taps);
    else
        hipLaunchKernelGGL((upfirdn2d_generic<false, float, float, float>), g, blk, lds, stream, (float*)y, (const float*)x, fir, p,
                           lds_taps);
    return ideas_launch_status();
}

extern "C" int ideas_upfirdn2d(void* y, const void* x, const float* fir, int B, int C, int in_h, int in_w, int out_h,
                               int out_w, int kh, int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0,
                               int pad_y0, float gain, int flip, int layout, int dtype, void* stream_) {
    return upfirdn2d_impl(y, x, fir, B, C, in_h, in_w, out_h, out_w, kh, kw, up_x, up_y, down_x, down_y, pad_x0, pad_y0, gain, flip,
                          layout, dtype, stream_, nullptr);
}

extern "C" int ideas_fir_up2_add(void* y, const void* x, const float* fir, const void* resid, int B, int C, int in_h, int in_w,
                                 int out_h, int out_w, int pad_x0, int pad_y0, float gain, int flip, int dtype, void* stream_) {
    if (!resid) return IDEAS_E_NULL;
    if (dtype != IDEAS_F32 && dtype != IDEAS_BF16) return IDEAS_E_UNSUPPORTED;       // (f16 / f64: ideas_upfirdn2d, then an add)
    return upfirdn2d_impl(y, x, fir, B, C, in_h, in_w, out_h, out_w, 4, 4, 2, 2, 1, 1, pad_x0, pad_y0, gain, flip, IDEAS_NHWC, dtype,
                          stream_, resid);
}
