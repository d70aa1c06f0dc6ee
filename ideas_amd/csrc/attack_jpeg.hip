// The JPEG FILE channel on the 8-bit container, device side: what libjpeg 6b / libjpeg-turbo with its defaults decodes from what it
// encoded -- 4:2:0 or 4:4:4, the integer "islow" DCT, the biased 2x2 chroma average, the triangle upsampler -- without the entropy
// coder.  All of it is int32, so the result is defined to the byte.  The model is stated step by step in include/ideas_hip.h ("The
// JPEG file channel") and restated in numpy by tests/jpegfile_ref.py, which tests/test_jpeg_file.py holds to Pillow's own bytes.
//
// The lane mapping, tables, colour conversion, row I/O, tile walk and the block's way through LDS are jpeg_block.hpp's, shared with
// attack.hip; the inverse pass and the triangle upsampler are jpeg_islow.hpp's, shared with the file reader (jpeg_decode.hip); this file
// holds the forward pass, the quantiser (islow_arith), the 4:2:0 average and the launchers.
//
// 4:2:0 takes two launches, because the upsampler needs one chroma sample of halo across block borders: chroma420_kernel loads 16x16
// pixels a block, converts, averages, round-trips Cb and Cr and writes the decoded half-resolution planes as bytes into the workspace;
// jpeg_file_kernel round-trips the luma, reads the workspace with clamped neighbours, upsamples, converts and stores.  4:4:4 and C = 1
// are jpeg_file_kernel alone.  DESIGN.md "Channel attacks".
#include "jpeg_islow.hpp"

namespace {

// FIRST: the row pass (results scaled up by 4); otherwise the column pass, which leaves 8 F
template <bool FIRST> __device__ __forceinline__ void fdct_pass(const int (&d)[8], int (&o)[8]) {
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int N = FIRST ? CONST_BITS - PASS1_BITS : CONST_BITS + PASS1_BITS;
    if constexpr (FIRST) {
        o[0] = (t10 + t11) << PASS1_BITS;
        o[4] = (t10 - t11) << PASS1_BITS;
    } else {
        o[0] = descale(t10 + t11, PASS1_BITS);
        o[4] = descale(t10 - t11, PASS1_BITS);
    }
    const int z1 = __mul24(t12 + t13, F_0_541);
    o[2] = descale(z1 + __mul24(t13, F_0_765), N);
    o[6] = descale(z1 + __mul24(t12, -F_1_847), N);
    int a4, a5, a6, a7;
    odd_part(t4, t5, t6, t7, a4, a5, a6, a7);
    o[7] = descale(a4, N); o[5] = descale(a5, N); o[3] = descale(a6, N); o[1] = descale(a7, N);
}

// sign(c) ((|c| + den / 2) / den) with den = 8 T: the quotient by the f32 reciprocal (numerator below 2^24, so off by one at most),
// put right by its remainder
__device__ __forceinline__ int quantise(int c, int den, float rden) {
    const int a = (c < 0 ? -c : c) + (den >> 1);
    int q = (int)((float)a * rden);
    const int rem = a - __mul24(q, den);
    q += (rem >= den ? 1 : 0) - (rem < 0 ? 1 : 0);
    return c < 0 ? -q : q;
}

// the IJG quality rule on Annex K: s_t the tables, s_d = 8 T and s_r = 1 / (8 T) for the quantiser; threads 0..127 of the workgroup
__device__ __forceinline__ void fill_tables(int (*s_t)[64], int (*s_d)[64], float (*s_r)[64], int qscale) {
    if (threadIdx.x < 128) {
        const int t = jpeg_table_entry(threadIdx.x, qscale);
        s_t[threadIdx.x >> 6][threadIdx.x & 63] = t;
        s_d[threadIdx.x >> 6][threadIdx.x & 63] = 8 * t;
        s_r[threadIdx.x >> 6][threadIdx.x & 63] = 1.0f / (float)(8 * t);
    }
}

// The integer model as block_roundtrip's arithmetic.  tq, dq, rq: the plane's T, 8 T and 1 / (8 T)
struct islow_arith {
    using T = int;
    const int *tq, *dq;
    const float* rq;
    __device__ __forceinline__ void rows_fwd(const int (&v)[8], int (&g)[8]) const {
        int a[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = v[j] - 128;
        fdct_pass<true>(a, g);
    }
    // a[u] becomes 8 F(u, r)
    __device__ __forceinline__ void cols_fwd(const int (&g)[8], int (&a)[8]) const { fdct_pass<false>(g, a); }
    __device__ __forceinline__ void quant_dequant(int (&a)[8], short (&qs)[8], int r) const {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int q = quantise(a[u], dq[u * 8 + r], rq[u * 8 + r]);
            qs[u] = (short)q;
            a[u] = __mul24(q, tq[u * 8 + r]);
        }
    }
    __device__ __forceinline__ void cols_inv(const int (&a)[8], int (&g)[8]) const { idct_pass<true>(a, g); }
    __device__ __forceinline__ void rows_inv(const int (&a)[8], int (&v)[8]) const {
        int g[8];
        idct_pass<false>(a, g);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = clamp_u8(g[j] + 128);
    }
};

// 4:2:0, launch one.  A wave owns 8 chroma blocks side by side; lane (block, r) owns chroma row 8 cby + r, 8 samples: 2 x 16 pixels.
// half: uint8 [B][2][ch][cw], the decoded Cb and Cr.  coef (or null): int16 [B][2][cbhn][cbwn][64].
template <bool VEC>
__global__ __launch_bounds__(256) void chroma420_kernel(unsigned char* __restrict__ half, short* __restrict__ coef,
                                                        const unsigned char* __restrict__ x, int H, int W, int qscale, int64_t ntiles) {
    __shared__ __attribute__((aligned(16))) int s_tile[2][4][8 * TILE_LD];        // [forward | inverse][wave][block][8][8]
    __shared__ int s_t[2][64], s_d[2][64];
    __shared__ float s_r[2][64];
    fill_tables(s_t, s_d, s_r, qscale);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, blk = lane & 7, r = lane >> 3;
    int* fw = &s_tile[0][wave][blk * TILE_LD];
    int* iv = &s_tile[1][wave][blk * TILE_LD];
    const int ch = (H + 1) >> 1, cw = (W + 1) >> 1;
    const int cbwn = (cw + 7) >> 3, cbhn = (ch + 7) >> 3, txn = (cbwn + 7) >> 3;

    for (int64_t t0 = tile_first(); t0 < ntiles; t0 += tile_step()) {
        const jpeg_tile t(t0, wave, lane, ntiles, txn, cbhn, cbwn);          // the walk over CHROMA blocks
        const int64_t b = t.b;
        const int cby = t.by, cbx = t.bx, cy = t.yy;
        const bool live = t.live;
        const int cyc = cy < ch ? cy : ch - 1;               // rows below the last chroma row repeat it: AFTER the average
        const int x0 = cbx * 16;                             // columns right of the image repeat the last column: BEFORE it

        int pl[2][8];                                        // Cb, Cr sums, then samples
#pragma unroll
        for (int k = 0; k < 8; ++k) pl[0][k] = pl[1][k] = (k & 1) ? 2 : 1;    // the bias: 1 on even, 2 on odd chroma columns
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int yy = 2 * cyc + dy < H ? 2 * cyc + dy : H - 1;          // an odd H repeats its last row
            const unsigned char* row = x + (b * H + yy) * W * 3;
#pragma unroll
            for (int hx = 0; hx < 2; ++hx) {
                int px[3][8];
                load8<3, VEC>(row, x0 + 8 * hx, W, px);
                if constexpr (VEC) {
                    if (hx == 1 && x0 + 8 >= W) {            // W % 16 == 8: the block's right half lies outside, the word held the left one
#pragma unroll
                        for (int j = 0; j < 7; ++j)
#pragma unroll
                            for (int c = 0; c < 3; ++c) px[c][j] = px[c][7];
                    }
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    pl[0][4 * hx + (j >> 1)] += cb_of(px[0][j], px[1][j], px[2][j]);
                    pl[1][4 * hx + (j >> 1)] += cr_of(px[0][j], px[1][j], px[2][j]);
                }
            }
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int k = 0; k < 8; ++k) pl[p][k] >>= 2;
            block_roundtrip(pl[p], islow_arith{s_t[1], s_d[1], s_r[1]}, fw, iv, r, coef && live,
                            coef + ((((b * 2 + p) * cbhn + cby) * cbwn + cbx) * 64 + r));
            if (live && cy < ch) {
                unsigned char* dst = half + ((b * 2 + p) * ch + cy) * cw + cbx * 8;
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (cbx * 8 + k < cw) dst[k] = (unsigned char)pl[p][k];
            }
        }
    }
}

// The luma (C = 1: the only plane) and, with SUB == 0 and C == 3, the full-resolution chroma round trip; with SUB == 2 the chroma comes
// from `half` (chroma420_kernel's bytes) through the upsampler.  VEC: W % 8 == 0, x and out 8-byte aligned, y 16-byte aligned.
template <int C, int SUB, bool VEC>
__global__ __launch_bounds__(256) void jpeg_file_kernel(unsigned char* __restrict__ out, float* __restrict__ y, short* __restrict__ coef_y,
                                                        short* __restrict__ coef_c, const unsigned char* __restrict__ half,
                                                        const unsigned char* __restrict__ x, int H, int W, int qscale, int64_t ntiles) {
    __shared__ __attribute__((aligned(16))) int s_tile[2][4][8 * TILE_LD];
    __shared__ int s_t[2][64], s_d[2][64];
    __shared__ float s_r[2][64];
    __shared__ float s_unit[256];                            // byte -> received f32
    fill_unit(s_unit);
    fill_tables(s_t, s_d, s_r, qscale);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, blk = lane & 7, r = lane >> 3;
    int* fw = &s_tile[0][wave][blk * TILE_LD];
    int* iv = &s_tile[1][wave][blk * TILE_LD];
    const int bwn = (W + 7) >> 3, bhn = (H + 7) >> 3, txn = (bwn + 7) >> 3;
    constexpr int NP = (C == 3 && SUB == 0) ? 3 : 1;         // planes that make the round trip here

    for (int64_t t0 = tile_first(); t0 < ntiles; t0 += tile_step()) {
        const jpeg_tile t(t0, wave, lane, ntiles, txn, bhn, bwn);
        const int64_t b = t.b;
        const int by = t.by, bx = t.bx, x0 = t.x0, yy = t.yy;
        const bool live = t.live;
        const int64_t row_in = (b * H + (yy < H ? yy : H - 1)) * W;   // replicated last row

        int pl[3][8];                                        // Y (Cb Cr), 0..255
        {
            int px[C][8];
            load8<C, VEC>(x + row_in * C, x0, W, px);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if constexpr (C == 3) {
                    pl[0][j] = luma_of(px[0][j], px[1][j], px[2][j]);
                    if constexpr (SUB == 0) {
                        pl[1][j] = cb_of(px[0][j], px[1][j], px[2][j]);
                        pl[2][j] = cr_of(px[0][j], px[1][j], px[2][j]);
                    }
                } else {
                    pl[0][j] = px[0][j];
                }
            }
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            short* const coef = p == 0 ? coef_y : coef_c;           // [B][1][bhn][bwn][64] and [B][2][bhn][bwn][64]
            const int64_t plane = p == 0 ? b : b * 2 + (p - 1);
            block_roundtrip(pl[p], islow_arith{s_t[p > 0], s_d[p > 0], s_r[p > 0]}, fw, iv, r, coef && live,
                            coef + (((plane * bhn + by) * bwn + bx) * 64 + r));
        }
        if constexpr (C == 3 && SUB == 2) {
            IDEAS_UPSAMPLE420_ROW(half, b, H, W, yy, bx, pl)
        }

        unsigned ob[8 * C];                                  // the bytes of this lane's row, pixel-major
        ycc_to_rgb<C>(pl, ob);
        if (live && yy < H) store8<C, VEC>(out, y, ((b * H + yy) * W + x0) * C, ob, x0, W, s_unit);
    }
}

unsigned grid_for(int64_t ntiles) {
    const int64_t grid = ideas_cdiv(ntiles, 4);
    return (unsigned)(grid > 16384 ? 16384 : grid);
}

template <int C, int SUB>
int launch_file(void* out, float* y, short* coef_y, short* coef_c, void* workspace, const void* x, int B, int H, int W, int quality,
                hipStream_t stream) {
    const int qscale = jpeg_qscale(quality);
    const bool x8 = W % 8 == 0 && ideas_aligned<8>(x);
    if constexpr (C == 3 && SUB == 2) {
        const int64_t ch = (H + 1) / 2, cw = (W + 1) / 2;
        const int64_t ntiles = (int64_t)B * ideas_cdiv(ch, 8) * ideas_cdiv(ideas_cdiv(cw, 8), 8);
        if (x8)
            hipLaunchKernelGGL((chroma420_kernel<true>), dim3(grid_for(ntiles)), dim3(256), 0, stream, (unsigned char*)workspace, coef_c,
                               (const unsigned char*)x, H, W, qscale, ntiles);
        else
            hipLaunchKernelGGL((chroma420_kernel<false>), dim3(grid_for(ntiles)), dim3(256), 0, stream, (unsigned char*)workspace, coef_c,
                               (const unsigned char*)x, H, W, qscale, ntiles);
        const int rc = ideas_launch_status();
        if (rc != IDEAS_OK) return rc;
    }
    const int64_t ntiles = (int64_t)B * ideas_cdiv(H, 8) * ideas_cdiv(ideas_cdiv(W, 8), 8);
    const bool vec = x8 && ideas_aligned<8>(out) && ideas_aligned16(y);
    if (vec)
        hipLaunchKernelGGL((jpeg_file_kernel<C, SUB, true>), dim3(grid_for(ntiles)), dim3(256), 0, stream, (unsigned char*)out, y, coef_y,
                           coef_c, (const unsigned char*)workspace, (const unsigned char*)x, H, W, qscale, ntiles);
    else
        hipLaunchKernelGGL((jpeg_file_kernel<C, SUB, false>), dim3(grid_for(ntiles)), dim3(256), 0, stream, (unsigned char*)out, y, coef_y,
                           coef_c, (const unsigned char*)workspace, (const unsigned char*)x, H, W, qscale, ntiles);
    return ideas_launch_status();
}

}  // namespace

extern "C" size_t ideas_jpeg_file_workspace_bytes(int B, int C, int H, int W, int subsampling) {
    if (B <= 0 || H <= 0 || W <= 0 || C != 3 || subsampling != 2) return 0;
    return (size_t)2 * (size_t)B * (size_t)((H + 1) / 2) * (size_t)((W + 1) / 2);
}

extern "C" int ideas_jpeg_file_roundtrip(void* out_u8, float* y, short* coef_y, short* coef_c, void* workspace, const void* x_u8, int B,
                                         int C, int H, int W, int quality, int subsampling, void* stream_) {
    if (!x_u8 || !out_u8) return IDEAS_E_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || (C != 1 && C != 3)) return IDEAS_E_SHAPE;
    if (quality < 1 || quality > 100) return IDEAS_E_UNSUPPORTED;
    if (subsampling != 0 && subsampling != 2) return IDEAS_E_UNSUPPORTED;
    if (!workspace && ideas_jpeg_file_workspace_bytes(B, C, H, W, subsampling) != 0) return IDEAS_E_NULL;
    hipStream_t stream = (hipStream_t)stream_;
    if (C == 1) return launch_file<1, 0>(out_u8, y, coef_y, nullptr, nullptr, x_u8, B, H, W, quality, stream);
    return subsampling == 2 ? launch_file<3, 2>(out_u8, y, coef_y, coef_c, workspace, x_u8, B, H, W, quality, stream)
                            : launch_file<3, 0>(out_u8, y, coef_y, coef_c, nullptr, x_u8, B, H, W, quality, stream);
}
