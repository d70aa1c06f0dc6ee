// What the two JPEG models of the 8-bit container share -- attack.hip's f32 baseline round trip and attack_jpeg.hip's libjpeg-exact
// integer one: the Annex K tables and the IJG quality rule, the fixed-point colour conversion both ways, a lane's 8-pixel row load and
// row store, the walk over tiles of 8 blocks, and the trip of one 8x8 block through two LDS tiles.  The arithmetic of a model (its
// 8-point transforms, its quantiser, its final rounding) stays in its own file, as the `Arith` of block_roundtrip.
//
// Lane mapping: eight lanes own one 8x8 block, one row of 8 samples each; a wave owns 8 blocks side by side (8 rows x 64 columns), lane
// = 8 * row + block, so that lanes 8 r .. 8 r + 7 read one contiguous run of 64 * C bytes of image row r.  DESIGN.md 3.15, 8.8.
#pragma once
#include "u8.hpp"

namespace {

// ISO/IEC 10918-1 Annex K, tables K.1 (luminance) and K.2 (chrominance), index 8 u + v
__device__ const unsigned char k_annex_k[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// The IJG quality rule.  Host side: the percentage that scales Annex K, from a quality of 1..100
inline int jpeg_qscale(int quality) { return quality < 50 ? 5000 / quality : 200 - 2 * quality; }
// device side: entry i (0..63 luminance, 64..127 chrominance) of the scaled tables, 1..255
__device__ __forceinline__ int jpeg_table_entry(int i, int qscale) {
    const int t = ((int)k_annex_k[i >> 6][i & 63] * qscale + 50) / 100;
    return t < 1 ? 1 : clamp_u8(t);
}

// RGB -> YCbCr in 16-bit fixed point (24-bit multiplies: the factors are below 2^17 and 2^8, the products exact)
__device__ __forceinline__ int luma_of(int R, int G, int Bl) { return (__mul24(19595, R) + __mul24(38470, G) + __mul24(7471, Bl) + 32768) >> 16; }
__device__ __forceinline__ int cb_of(int R, int G, int Bl) {
    return (__mul24(-11059, R) - __mul24(21709, G) + __mul24(32768, Bl) + (128 << 16) + 32767) >> 16;
}
__device__ __forceinline__ int cr_of(int R, int G, int Bl) {
    return (__mul24(32768, R) - __mul24(27439, G) - __mul24(5329, Bl) + (128 << 16) + 32767) >> 16;
}

// and back, for a lane's eight pixels: planes Y (Cb Cr) of 0..255 -> the bytes of its row, pixel-major.  C = 1: the plane itself
template <int C, int P> __device__ __forceinline__ void ycc_to_rgb(const int (&pl)[P][8], unsigned (&ob)[8 * C]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if constexpr (C == 3) {
            const int Y = pl[0][j], cb = pl[1][j] - 128, cr = pl[2][j] - 128;
            ob[3 * j] = (unsigned)clamp_u8(Y + ((__mul24(91881, cr) + 32768) >> 16));
            ob[3 * j + 1] = (unsigned)clamp_u8(Y + ((__mul24(-22554, cb) - __mul24(46802, cr) + 32768) >> 16));
            ob[3 * j + 2] = (unsigned)clamp_u8(Y + ((__mul24(116130, cb) + 32768) >> 16));
        } else {
            ob[j] = (unsigned)pl[0][j];
        }
    }
}

// 8 pixels of one image row (row = x + row offset in bytes) from column x0 on.  VEC (W % 8 == 0, 8-byte aligned rows): C 8-byte
// words, a lane past the row reads its last 8 pixels; otherwise byte by byte with the last column replicated.
template <int C, bool VEC> __device__ __forceinline__ void load8(const unsigned char* __restrict__ row, int x0, int W, int (&px)[C][8]) {
    if constexpr (VEC) {
        const int xl = x0 < W ? x0 : W - 8;
        unsigned w[2 * C];
        const uint2* p = reinterpret_cast<const uint2*>(row + (int64_t)xl * C);
#pragma unroll
        for (int k = 0; k < C; ++k) { const uint2 v = p[k]; w[2 * k] = v.x; w[2 * k + 1] = v.y; }
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int c = 0; c < C; ++c) px[c][j] = (int)byte_of(w, j * C + c);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int xc = x0 + j < W ? x0 + j : W - 1;
            const unsigned char* p = row + (int64_t)xc * C;
#pragma unroll
            for (int c = 0; c < C; ++c) px[c][j] = p[c];
        }
    }
}

// the 8 pixels ob of a lane's row from column x0 on to out and y (o: the byte offset of the first).  VEC: C 8-byte words and 2 C
// float4 (out 8-byte, y 16-byte aligned, W % 8 == 0); otherwise the pixels inside the row, byte by byte
template <int C, bool VEC>
__device__ __forceinline__ void store8(unsigned char* __restrict__ out, float* __restrict__ y, int64_t o, const unsigned (&ob)[8 * C],
                                       int x0, int W, const float* s_unit) {
    store_bytes<8 * C, VEC ? 8 : 0, C>(out, y, o, ob, W - x0, unit_table{s_unit});
}

constexpr int TILE_LD = 72;        // elements from one block's 8x8 LDS tile to the next: the column reads of a half-wave fall on 32 banks

// The tile walk.  A workgroup is four waves, a wave takes one tile (8 blocks side by side) a trip, and block_roundtrip holds two
// workgroup barriers: every wave of a workgroup makes the same number of trips, and a wave past the last tile repeats it without
// stores (live = false).  for (int64_t t0 = tile_first(); t0 < ntiles; t0 += tile_step()) { const jpeg_tile t(t0, ...); ... }
__device__ __forceinline__ int64_t tile_first() { return (int64_t)blockIdx.x * 4; }
__device__ __forceinline__ int64_t tile_step() { return (int64_t)gridDim.x * 4; }

struct jpeg_tile {
    int64_t b;                     // image
    int by, bx;                    // this lane's block
    int x0, yy;                    // its first sample column 8 bx and this lane's sample row 8 by + r
    bool live;                     // the block exists and the wave's tile is its own: stores allowed
    // ntiles = images x bhn x txn tiles, txn = ceil(bwn / 8); lane = 8 r + (block of the tile)
    __device__ __forceinline__ jpeg_tile(int64_t t0, int wave, int lane, int64_t ntiles, int txn, int bhn, int bwn) {
        const bool live_tile = t0 + wave < ntiles;
        const int64_t t = live_tile ? t0 + wave : ntiles - 1;
        const int tx = (int)(t % txn);
        by = (int)((t / txn) % bhn);
        b = t / txn / bhn;
        bx = tx * 8 + (lane & 7);
        live = live_tile && bx < bwn;
        x0 = bx * 8;
        yy = by * 8 + (lane >> 3);
    }
};

__device__ __forceinline__ float4 vec4(float a, float b, float c, float d) { return make_float4(a, b, c, d); }
__device__ __forceinline__ int4 vec4(int a, int b, int c, int d) { return make_int4(a, b, c, d); }

// One plane's 8x8 block through forward transform, quantiser, dequantiser and inverse: v = this lane's row r of samples 0..255 in, the
// decoded row out.  The row pass runs in registers with lane = (block, row r); the block is transposed through the wave-private LDS
// tile fw (two 16-byte stores, column reads at stride 8 inside a block, TILE_LD between blocks); the column pass, the quantiser and the
// dequantiser run in registers with lane = (block, column r); the inverse goes the same way back through iv.  keep: store the
// quantised coefficients to cdst, the block's 64 + r (the condition apart from the pointer, which is then not looked at: a pointer that
// is null for "no" costs a 64-bit select and compare a plane).  Two workgroup barriers: every wave of the workgroup calls this the same
// number of times.
// Arith: the model's element type T and its five steps --
//   rows_fwd(v, g)        samples 0..255 -> the row pass
//   cols_fwd(g, a)        the column pass
//   quant_dequant(a, qs, r)   a[u] = coefficient (u, r) -> qs[u] its quantised value, a[u] the dequantised one
//   cols_inv(a, g), rows_inv(a, v)   the inverse passes, the last with the final rounding to a byte
template <class Arith>
__device__ __forceinline__ void block_roundtrip(int (&v)[8], const Arith& ar, typename Arith::T* fw, typename Arith::T* iv, int r,
                                                bool keep, short* __restrict__ cdst) {
    using T = typename Arith::T;
    using T4 = decltype(vec4(T(), T(), T(), T()));
    T a[8], g[8];
    ar.rows_fwd(v, g);
    reinterpret_cast<T4*>(fw + r * 8)[0] = vec4(g[0], g[1], g[2], g[3]);
    reinterpret_cast<T4*>(fw + r * 8)[1] = vec4(g[4], g[5], g[6], g[7]);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) g[i] = fw[i * 8 + r];
    ar.cols_fwd(g, a);
    short qs[8];
    ar.quant_dequant(a, qs, r);
    if (keep) {
#pragma unroll
        for (int u = 0; u < 8; ++u) cdst[u * 8] = qs[u];
    }
    ar.cols_inv(a, g);
#pragma unroll
    for (int i = 0; i < 8; ++i) iv[i * 8 + r] = g[i];
    __syncthreads();
    {
        const T4 v0 = reinterpret_cast<const T4*>(iv + r * 8)[0], v1 = reinterpret_cast<const T4*>(iv + r * 8)[1];
        a[0] = v0.x; a[1] = v0.y; a[2] = v0.z; a[3] = v0.w; a[4] = v1.x; a[5] = v1.y; a[6] = v1.z; a[7] = v1.w;
    }
    ar.rows_inv(a, v);
}

}  // namespace
