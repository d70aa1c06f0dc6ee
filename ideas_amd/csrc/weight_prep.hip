// Derived weights: the bf16 forms the MFMA kernels read instead of the f32 parameter, remade after every optimiser step.
//
//   IDEAS_PREP_B3_SPLIT   split-bf16 planes [3][K/16][Cout][16] of conv_b3.hip, K-step = (ci/16, ty, tx): taps innermost, so the B tile
//                         of a K-step is one contiguous 4 KB block;  w = hi + mid + lo EXACTLY (b3.hpp::split4)
//   IDEAS_PREP_BF16_PACK  bf16 pack [K/32][Cout][32] of conv_bf16.hip, K-step = (ci/32, ty, tx), 16-byte chunk c of row n stored at
//                         c ^ ((n >> 2) & 3) (the kernel's LDS swizzle, so its DMA copies linearly).  With `scale` (float [B][Cin]): B
//                         packs, pack b = bf16(w[n][k] * scale[b][ci(k)]) -- the reference's per-sample modulated weights
//                         (stylegan2/model.py:240-248), for the life of one launch
//   IDEAS_PREP_B3_WINO    Winograd F(2,3)-transformed AND split planes [4 v][3][3*C/16][N][16] of conv_b3_wino.hip, step = (c/16, ky)
//
// Every form reads element (n, ty, tx, c) of the launch's [N][TY][TX][C] matrix straight from the PARAMETER, at
// w[n*sn + ty*sty + tx*stx + c*sc] (f32 elements): the forward matrix of an [O,I,KH,KW] tensor of any strides, the phase-sliced
// transposed matrix of an input gradient or the matrix of a transposed conv, so no permuted / sliced f32 copy is materialised first.
//
// One job = one ideas_prep_desc.  ideas_weight_prep_plan is the ONLY place that knows a form's channel granularity and element
// count, when the 16-byte read path applies (`unit`) and how many blocks a job gets (`nblocks`); ideas_weight_prep runs one job from
// a host descriptor, ideas_weight_prep_batched a device table of planned jobs (~390 launches of 5-25 us per iteration otherwise,
// most too small to fill the chip), and the single-tensor entry points of include/ideas_hip.h fill a descriptor and take the same
// path.  Per form there is one per-element body, so every route gives the same bytes.
// (the splits keep the plain f32 operators, as in conv_b3.hip and conv_b3_wino.hip where these kernels came from)
#define B3_UNPACK_F32 0
#include "b3.hpp"
#include "conv_launch.hpp"

namespace {

constexpr int prep_vec(int op) { return op == IDEAS_PREP_BF16_PACK ? 8 : 4; }      // channels per work item; a K-step holds four items

// Work item i of an [N][TY][TX][C] matrix read VEC channels at a time through the strides of `d`: its (n, tap, c) and the VEC values.
// UNIT (unit channel stride, 16-byte aligned rows): consecutive threads read consecutive 16-byte pieces of one (n, tap) row;
// otherwise consecutive threads take consecutive n (the contiguous index of a transposed read) of one (tap, VEC-channel chunk).
template <int VEC, bool UNIT>
__device__ __forceinline__ void prep_item(const ideas_prep_desc& d, int64_t i, int& n, int& tap, int& c, float (&v)[VEC]) {
    const int N = d.a[0], TX = d.a[2], cv = d.a[3] / VEC, ntaps = d.a[1] * TX;
    if (UNIT) {
        c = (int)(i % cv) * VEC;
        tap = (int)((i / cv) % ntaps);
        n = (int)(i / ((int64_t)cv * ntaps));
    } else {
        n = (int)(i % N);
        c = (int)((i / N) % cv) * VEC;
        tap = (int)(i / ((int64_t)N * cv));
    }
    const int ty = tap / TX, tx = tap - ty * TX;
    const float* src = d.w + n * d.s[0] + ty * d.s[1] + tx * d.s[2] + c * d.s[3];
#pragma unroll
    for (int j = 0; j < VEC; j += 4) {
        const float4 u = UNIT ? *reinterpret_cast<const float4*>(src + j)
                              : make_float4(src[j * d.s[3]], src[(j + 1) * d.s[3]], src[(j + 2) * d.s[3]], src[(j + 3) * d.s[3]]);
        v[j] = u.x; v[j + 1] = u.y; v[j + 2] = u.z; v[j + 3] = u.w;
    }
}

// b3 split / bf16 pack: what the two do with an item's values, and where they store them
template <int OP, bool UNIT>
__device__ __forceinline__ void prep_rows(const ideas_prep_desc& d, const float* __restrict__ scale, int b, int64_t bid, int64_t nblk) {
    constexpr int VEC = prep_vec(OP);
    const int Cout = d.a[0], Cin = d.a[3], ntaps = d.a[1] * d.a[2];
    const int64_t items = (int64_t)Cout * ntaps * (Cin / VEC);          // = 16-byte (pack) / 8-byte (one plane) units of the destination
    const float* sb = scale ? scale + (int64_t)b * Cin : nullptr;
    for (int64_t i = bid * 256 + threadIdx.x; i < items; i += nblk * 256) {
        int n, tap, ci;
        float v[VEC];
        prep_item<VEC, UNIT>(d, i, n, tap, ci, v);
        const int step = ci / (4 * VEC) * ntaps + tap;                  // K-steps run over the taps of one chunk, then the next chunk
        const int q = (ci / VEC) & 3;
        const int64_t row = ((int64_t)step * Cout + n) * 4;
        if constexpr (OP == IDEAS_PREP_B3_SPLIT) {
            const Split4 s = split4(make_float4(v[0], v[1], v[2], v[3]));
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) ((uint2*)d.dst)[pl * items + row + q] = s.p[pl];
        } else {
            if (sb) {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] *= sb[ci + j];
            }
            ((uint4*)d.dst)[b * items + row + (q ^ ((n >> 2) & 3))] =
                make_uint4(ideas_pk_bf16(v[0], v[1]), ideas_pk_bf16(v[2], v[3]), ideas_pk_bf16(v[4], v[5]), ideas_pk_bf16(v[6], v[7]));
        }
    }
}

// Winograd planes: a = (N, C), element (n, ky, kx, c) at w[base + n*sn + ky*sky + kx*skx + c*sc], s = (sn, sky, skx, sc, base)
//   forward : n = o, c = i on the OHWI parameter          (sn = 9I, sky = 3I, skx = I, sc = 1, base = 0)
//   dgrad   : n = i, c = o, taps flipped, same parameter  (sn = 1, sky = -3I, skx = -I, sc = 9I, base = 8I)
// An item is four channels of one (n, ky) and reads their three kx taps (element reads: no 16-byte path).
__device__ __forceinline__ void prep_wino(const ideas_prep_desc& d, int64_t bid, int64_t nblk) {
    const int N = d.a[0], C = d.a[1];
    const float* __restrict__ w = d.w + d.s[4];
    uint2* __restrict__ dst = (uint2*)d.dst;
    const int64_t total = (int64_t)N * 3 * (C / 4);
    const int64_t plane = total;                          // uint2 units per (v, plane)
    for (int64_t i = bid * 256 + threadIdx.x; i < total; i += nblk * 256) {
        const int c = (int)(i % (C / 4)) * 4;
        const int ky = (int)((i / (C / 4)) % 3);
        const int n = (int)(i / (3 * (C / 4)));
        float wk[3][4];
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
            for (int e = 0; e < 4; ++e) wk[kx][e] = w[n * d.s[0] + ky * d.s[1] + kx * d.s[2] + (c + e) * d.s[3]];
        // The transformed weights are the same for every pixel of every sample, so an error in them is a COHERENT error of the
        // outputs: it does not average out in the backward's sums over 65 536 pixels (weight gradient, style / demodulation dot
        // products) the way per-pixel rounding does.  Rounding U twice in f32 ((w0 + w2) + w1, 1.2e-7 relative) made G's late-layer
        // gradients sit 4x further from f64 than stock f32 arithmetic (tests/test_nets_gpu.py::test_full_width_gradients_vs_oracle);
        // the sums are exact in double, and the three planes are cut from the double: hi + mid + lo = U to ~2^-26.
        double u[4][4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double s = (double)wk[0][e] + (double)wk[2][e];
            u[0][e] = wk[0][e];
            u[1][e] = (s + (double)wk[1][e]) * 0.5;
            u[2][e] = (s - (double)wk[1][e]) * 0.5;
            u[3][e] = wk[2][e];
        }
        const int step = (c >> 4) * 3 + ky;
        const int64_t o = ((int64_t)step * N + n) * 4 + ((c & 15) >> 2);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            Split4 s;
            split2d(u[v][0], u[v][1], s.p[0].x, s.p[1].x, s.p[2].x);
            split2d(u[v][2], u[v][3], s.p[0].y, s.p[1].y, s.p[2].y);
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) dst[(v * 3 + pl) * plane + o] = s.p[pl];
        }
    }
}

// job of this block in a table sorted by block0: block-uniform binary search over the first-block prefix
__device__ __forceinline__ const ideas_prep_desc* prep_lookup(const ideas_prep_desc* tbl, int n, int& local, int& nblk) {
    int lo = 0, hi = n - 1;
    const int b = (int)blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tbl[mid].block0 <= b) lo = mid; else hi = mid - 1;
    }
    local = b - tbl[lo].block0;
    nblk = tbl[lo].nblocks;
    return tbl + lo;
}

// One kernel per form and descriptor source.  BATCHED: the job is looked up in the table `tbl` of `n` jobs (no scale); otherwise it is
// `one`, the grid is (one.nblocks, packs) and blockIdx.y selects the per-sample pack.
template <int OP, bool BATCHED>
__global__ __launch_bounds__(256) void weight_prep_kernel(ideas_prep_desc one, const ideas_prep_desc* __restrict__ tbl, int n,
                                                          const float* __restrict__ scale) {
    int local = blockIdx.x, nblk = gridDim.x;
    if (BATCHED) one = *prep_lookup(tbl, n, local, nblk);
    const float* sc = BATCHED ? nullptr : scale;
    if constexpr (OP == IDEAS_PREP_B3_WINO) prep_wino(one, local, nblk);
    else if (one.unit) prep_rows<OP, true>(one, sc, blockIdx.y, local, nblk);
    else prep_rows<OP, false>(one, sc, blockIdx.y, local, nblk);
}

template <bool BATCHED>
int prep_launch(int op, const ideas_prep_desc& one, const ideas_prep_desc* tbl, int n, const float* scale, dim3 grid, void* stream) {
    const auto go = [&](auto form) {
        hipLaunchKernelGGL((weight_prep_kernel<decltype(form)::value, BATCHED>), grid, dim3(256), 0, (hipStream_t)stream, one, tbl, n, scale);
    };
    switch (op) {
        case IDEAS_PREP_B3_SPLIT: go(std::integral_constant<int, IDEAS_PREP_B3_SPLIT>{}); break;
        case IDEAS_PREP_B3_WINO: go(std::integral_constant<int, IDEAS_PREP_B3_WINO>{}); break;
        case IDEAS_PREP_BF16_PACK: go(std::integral_constant<int, IDEAS_PREP_BF16_PACK>{}); break;
        default: return IDEAS_E_UNSUPPORTED;
    }
    return ideas_launch_status();
}

// ideas_weight_prep, and the single-tensor entry points behind it.  `dense`: the caller promises a 16-byte aligned dense matrix
// (ideas_b3_split_weights / ideas_bf16_pack_weights), which always takes the 16-byte read path.
int prep_run(ideas_prep_desc d, int op, const float* in_scale, int B, bool dense, void* stream) {
    if (!d.dst || !d.w) return IDEAS_E_NULL;
    int64_t elems;
    const int rc = ideas_weight_prep_plan(&d, op, &elems);
    if (rc != IDEAS_OK && rc != IDEAS_E_ALIGN) return rc;
    if (in_scale && op != IDEAS_PREP_BF16_PACK) return IDEAS_E_UNSUPPORTED;
    if (B <= 0 || B > 65535) return IDEAS_E_SHAPE;
    if (rc || !ideas_aligned16(d.dst) || (dense && !ideas_aligned16(d.w)) || (in_scale && !ideas_aligned16(in_scale))) return IDEAS_E_ALIGN;
    if (!in_scale && B != 1) return IDEAS_E_SHAPE;
    return prep_launch<false>(op, d, nullptr, 0, in_scale, dim3(d.nblocks, B), stream);
}

ideas_prep_desc prep_desc(void* dst, const void* w, int a0, int a1, int a2, int a3, int64_t s0, int64_t s1, int64_t s2, int64_t s3,
                          int64_t s4 = 0) {
    return ideas_prep_desc{dst, (const float*)w, {s0, s1, s2, s3, s4}, {a0, a1, a2, a3}, 0, 0, 0, 0};
}

}  // namespace

extern "C" int ideas_sizeof_prep_desc(void) { return (int)sizeof(ideas_prep_desc); }

extern "C" int ideas_weight_prep_plan(ideas_prep_desc* d, int op, int64_t* dst_elems) {
    if (!d || !dst_elems) return IDEAS_E_NULL;
    if (op != IDEAS_PREP_B3_SPLIT && op != IDEAS_PREP_B3_WINO && op != IDEAS_PREP_BF16_PACK) return IDEAS_E_UNSUPPORTED;
    const bool wino = op == IDEAS_PREP_B3_WINO;                      // a = (N, C), three ky taps; else a = (Cout, TY, TX, Cin)
    const int vec = prep_vec(op), planes = wino ? 12 : op == IDEAS_PREP_B3_SPLIT ? 3 : 1;
    for (int j = 0; j < (wino ? 2 : 4); ++j)
        if (d->a[j] <= 0) return IDEAS_E_SHAPE;
    const int C = d->a[wino ? 1 : 3];
    if (C % (4 * vec)) return IDEAS_E_ALIGN;                         // a K-step is four work items of `vec` channels
    const int64_t elems = (int64_t)d->a[0] * (wino ? 3 : (int64_t)d->a[1] * d->a[2]) * C;
    *dst_elems = planes * elems;
    // the 16-byte read path: unit channel stride, and every (n, ty, tx) row starts on a 16-byte boundary
    d->unit = !wino && d->s[3] == 1 && ideas_aligned16(d->w) && d->s[0] % 4 == 0 && d->s[1] % 4 == 0 && d->s[2] % 4 == 0;
    // grid-stride over the work items: a block per 256 of them, at most 2048 blocks
    const int64_t items = elems / vec;
    d->nblocks = (int)(items / 256 + 1 < 2048 ? items / 256 + 1 : 2048);
    return IDEAS_OK;
}

extern "C" int ideas_weight_prep(const ideas_prep_desc* host_desc, int op, const float* in_scale, int B, void* stream) {
    if (!host_desc) return IDEAS_E_NULL;
    return prep_run(*host_desc, op, in_scale, B, false, stream);
}

extern "C" int ideas_weight_prep_batched(const ideas_prep_desc* table, int n, int op, int total_blocks, void* stream) {
    if (!table) return IDEAS_E_NULL;
    if (n <= 0 || total_blocks <= 0) return IDEAS_E_SHAPE;
    return prep_launch<true>(op, ideas_prep_desc{}, table, n, nullptr, dim3(total_blocks), stream);
}

// The single-tensor entry points: a descriptor each.  A dense [Cout][K] matrix is TY = 1, TX = K / Cin at strides (K, K, Cin, 1).
extern "C" int ideas_b3_split_weights(void* planes, const void* wmat, int Cout, int K, int Cin, void* stream) {
    if (!planes || !wmat) return IDEAS_E_NULL;
    if (Cout <= 0 || K <= 0 || Cin <= 0 || K % Cin) return IDEAS_E_SHAPE;
    return prep_run(prep_desc(planes, wmat, Cout, 1, K / Cin, Cin, K, K, Cin, 1), IDEAS_PREP_B3_SPLIT, nullptr, 1, true, stream);
}

extern "C" int ideas_b3_split_weights_strided(void* planes, const float* w, int Cout, int TY, int TX, int Cin, int64_t sn, int64_t sty,
                                              int64_t stx, int64_t sc, void* stream) {
    return prep_run(prep_desc(planes, w, Cout, TY, TX, Cin, sn, sty, stx, sc), IDEAS_PREP_B3_SPLIT, nullptr, 1, false, stream);
}

extern "C" int ideas_b3_wino_split_weights(void* planes, const void* w, int N, int C, int64_t sn, int64_t sky, int64_t skx,
                                           int64_t sc, int64_t base, void* stream) {
    return prep_run(prep_desc(planes, w, N, C, 0, 0, sn, sky, skx, sc, base), IDEAS_PREP_B3_WINO, nullptr, 1, false, stream);
}

extern "C" int ideas_bf16_pack_weights(void* pack, const void* wmat, const float* in_scale, int B, int Cout, int K, int Cin,
                                       void* stream) {
    if (!pack || !wmat) return IDEAS_E_NULL;
    if (Cout <= 0 || K <= 0 || Cin <= 0 || K % Cin) return IDEAS_E_SHAPE;
    return prep_run(prep_desc(pack, wmat, Cout, 1, K / Cin, Cin, K, K, Cin, 1), IDEAS_PREP_BF16_PACK, in_scale, B, true, stream);
}

extern "C" int ideas_bf16_pack_weights_strided(void* pack, const float* w, const float* in_scale, int B, int Cout, int TY, int TX,
                                               int Cin, int64_t sn, int64_t sty, int64_t stx, int64_t sc, void* stream) {
    return prep_run(prep_desc(pack, w, Cout, TY, TX, Cin, sn, sty, stx, sc), IDEAS_PREP_BF16_PACK, in_scale, B, false, stream);
}
