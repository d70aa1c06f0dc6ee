// Spatial channel attacks on the 8-bit container, device side: one separable integer resampling kernel (Pillow's 8-bit BILINEAR
// resize and a Gaussian blur are both "each output index is a short weighted window of input indices") and a 3x3 / 5x5 median.  The
// model is stated step by step in include/ideas_hip.h ("Spatial channel attacks") and restated in numpy by tests/spatial_ref.py;
// everything is integer arithmetic, so the tests compare byte for byte.  DESIGN.md "Spatial channel attacks".
//
// Both kernels see a row of the image as W * C BYTES and give a thread four consecutive bytes of an output row (one 4-byte word of out,
// one float4 of y): byte q of the row is channel q % C of pixel q / C, and a tile starts at a multiple of 64 pixels, so a thread's word
// is 4-byte aligned in the row whatever C is.  Every LDS array is made of such words: lanes next to each other read and write words
// next to each other (consecutive banks), no lane touches a single byte of LDS.
#include "u8.hpp"

namespace {

constexpr int KMAX = IDEAS_RESAMPLE_KMAX;
constexpr int TW = 64;                                       // pixels across a tile: TW * C / 4 words a row
constexpr int TH = 32;                                       // output rows of a resampling tile
constexpr int LDS_ROWS = 160;                                // rows of the horizontal pass's result a tile may keep: 30 KiB at C = 3
constexpr int IN_WORDS = 2048;                               // words of input rows staged at a time for the horizontal pass: 8 KiB
constexpr int VK_LD = KMAX + 1;                              // ints from one output row's vertical coefficients to the next (odd)
constexpr int MTH = 16;                                      // output rows of a median tile

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the end of a pass: the sum (which started at 2^21) as a signed 32-bit integer, >> 22, clamped to a byte
__device__ __forceinline__ unsigned pass_byte(unsigned s) { return (unsigned)clamp_u8((int)s >> 22); }

// ---- resampling -------------------------------------------------------------------------------------------------------------------
// word d of the tile's part of the horizontal pass of one input row: four bytes, each its own pixel's window.  src holds the row's
// bytes from byte `sub` on (the row in HBM: sub = 0; its staged part in LDS: where that part begins).
// s_hlo [TW] and s_hkk [hk][TW] are the tile's columns of the tables (tap-major: lanes read consecutive banks).
template <int C>
__device__ __forceinline__ unsigned hpass_word(const unsigned char* src, int64_t sub, int W, int d, int hk, const int* s_hlo,
                                               const int* s_hkk) {
    unsigned word = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int q = 4 * d + e, pl = q / C, ch = q % C;
        const int lo = s_hlo[pl];
        unsigned s = 1u << 21;
        for (int j = 0; j < hk; ++j) {
            const int xi = clampi(lo + j, 0, W - 1);
            s += (unsigned)s_hkk[j * TW + pl] * (unsigned)src[(int64_t)xi * C + ch - sub];
        }
        word |= pass_byte(s) << (8 * e);
    }
    return word;
}

// A workgroup owns TH x TW output pixels.  It runs the horizontal pass for the input rows r0 .. r1 its rows' windows reach, into LDS
// as bytes, then the vertical pass out of LDS.  The horizontal pass reads its input out of LDS too: the bytes x0 .. x1 of a row that
// the tile's columns reach are staged a few rows at a time (IN_WORDS words; as 4-byte words when x and its rows are 4-byte aligned --
// vin --, byte by byte otherwise), because a window starts at any byte and a lane would otherwise fetch every tap from HBM by itself.
// A tile whose windows reach more than LDS_ROWS rows, or more than IN_WORDS words of one row (no table of op/resample.py does; a
// hand-made one may), takes the same sums from x directly, the horizontal pass recomputed per vertical tap: the same bytes.
// A direction without tables is the identity table lo[i] = i, kk = 2^22, ksize 1: (2^21 + 2^22 p) >> 22 == p.
template <int C, bool VEC>
__global__ __launch_bounds__(256) void resample_kernel(unsigned char* __restrict__ out, float* __restrict__ y,
                                                       const unsigned char* __restrict__ x, int H, int W, int H2, int W2,
                                                       const int* __restrict__ h_lo, const int* __restrict__ h_kk, int hk,
                                                       const int* __restrict__ v_lo, const int* __restrict__ v_kk, int vk, int tyn,
                                                       int txn, int64_t ntiles, bool vin) {
    constexpr int TWD = TW * C / 4;
    __shared__ unsigned s_rows[LDS_ROWS * TWD], s_in[IN_WORDS];
    __shared__ int s_hkk[KMAX * TW], s_vkk[TH * VK_LD], s_hlo[TW], s_vlo[TH];
    __shared__ float s_unit[256];
    const int tid = threadIdx.x;
    fill_unit(s_unit);

    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int tx = (int)(tile % txn), ty = (int)((tile / txn) % tyn);
        const int64_t b = tile / txn / tyn;
        const int ox0 = tx * TW, oy0 = ty * TH;
        const int tw = W2 - ox0 < TW ? W2 - ox0 : TW, th = H2 - oy0 < TH ? H2 - oy0 : TH;
        __syncthreads();                                     // the tile before is read; (first trip: s_unit is written)
        // the tile's part of the tables.  lo is brought into [-KMAX, n_in - 1] first: below and above, every lo + j clamps to the same
        // index as at the bound, and lo + j cannot overflow.  A column past the image repeats the last one (its bytes are not stored).
        for (int i = tid; i < TW * hk; i += 256) {
            const int pl = i % TW, j = i / TW, ox = ox0 + pl < W2 ? ox0 + pl : W2 - 1;
            s_hkk[j * TW + pl] = h_kk ? h_kk[(int64_t)ox * hk + j] : (1 << 22);
        }
        if (tid < TW) {
            const int ox = ox0 + tid < W2 ? ox0 + tid : W2 - 1;
            s_hlo[tid] = clampi(h_lo ? h_lo[ox] : ox, -KMAX, W - 1);
        }
        for (int i = tid; i < th * vk; i += 256) {
            const int r = i / vk, j = i % vk;
            s_vkk[r * VK_LD + j] = v_kk ? v_kk[(int64_t)(oy0 + r) * vk + j] : (1 << 22);
        }
        if (tid < th) s_vlo[tid] = clampi(v_lo ? v_lo[oy0 + tid] : oy0 + tid, -KMAX, H - 1);
        __syncthreads();

        int r0 = H - 1, r1 = 0;                              // the input rows the tile's windows reach, after clamping
        for (int r = 0; r < th; ++r) {
            const int a = clampi(s_vlo[r], 0, H - 1), z = clampi(s_vlo[r] + vk - 1, 0, H - 1);
            r0 = a < r0 ? a : r0;
            r1 = z > r1 ? z : r1;
        }
        int x0 = W - 1, x1 = 0;                              // and the input columns
        for (int pl = 0; pl < TW; ++pl) {
            const int a = clampi(s_hlo[pl], 0, W - 1), z = clampi(s_hlo[pl] + hk - 1, 0, W - 1);
            x0 = a < x0 ? a : x0;
            x1 = z > x1 ? z : x1;
        }
        const int nrows = r1 - r0 + 1;
        const unsigned char* xb = x + b * H * W * C;
        const int64_t rowb = (int64_t)W * C;
        const int64_t sb0 = ((int64_t)x0 * C) & ~(int64_t)3;                     // the staged part of a row: from this byte on,
        const int64_t nw64 = (((int64_t)x1 + 1) * C - sb0 + 3) >> 2;             // this many words (vin: it ends inside the row)
        const bool fits = nrows <= LDS_ROWS && nw64 <= IN_WORDS;                 // the same for every thread of the workgroup
        if (fits) {
            const int nwords = (int)nw64, chunk = IN_WORDS / nwords;
            for (int c0 = 0; c0 < nrows; c0 += chunk) {
                const int rc = nrows - c0 < chunk ? nrows - c0 : chunk;
                if (c0) __syncthreads();                     // the rows staged before are read
                for (int i = tid; i < rc * nwords; i += 256) {
                    const int rl = i / nwords, k = i % nwords;
                    const unsigned char* xr = xb + (r0 + c0 + rl) * rowb;
                    const int64_t n = sb0 + 4 * k;
                    unsigned w = 0;
                    if (vin) {
                        w = *reinterpret_cast<const unsigned*>(xr + n);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (n + e < rowb) w |= (unsigned)xr[n + e] << (8 * e);
                    }
                    s_in[i] = w;
                }
                __syncthreads();
                for (int i = tid; i < rc * TWD; i += 256) {
                    const int rl = i / TWD, d = i % TWD;
                    s_rows[c0 * TWD + i] = hpass_word<C>(reinterpret_cast<const unsigned char*>(s_in + rl * nwords), sb0, W, d, hk, s_hlo, s_hkk);
                }
            }
            __syncthreads();
        }
        for (int i = tid; i < th * TWD; i += 256) {
            const int orow = i / TWD, d = i % TWD;
            const int nvalid = tw * C - 4 * d;               // bytes of this word inside the image
            if (nvalid <= 0) continue;
            const int lo = s_vlo[orow];
            unsigned s[4] = {1u << 21, 1u << 21, 1u << 21, 1u << 21};
            for (int j = 0; j < vk; ++j) {
                const int row = clampi(lo + j, 0, H - 1);
                const unsigned w = fits ? s_rows[(row - r0) * TWD + d] : hpass_word<C>(xb + row * rowb, 0, W, d, hk, s_hlo, s_hkk);
                const unsigned k = (unsigned)s_vkk[orow * VK_LD + j];
#pragma unroll
                for (int e = 0; e < 4; ++e) s[e] += k * ((w >> (8 * e)) & 0xffu);
            }
            const unsigned ob[4] = {pass_byte(s[0]), pass_byte(s[1]), pass_byte(s[2]), pass_byte(s[3])};
            const int64_t o = ((b * H2 + oy0 + orow) * W2 + ox0) * C + 4 * d;
            store_bytes<4, VEC ? 4 : 0>(out, y, o, ob, nvalid, unit_table{s_unit});    // VEC: nvalid is 4 in every word
        }
    }
}

static unsigned tile_grid(int64_t ntiles) { return (unsigned)(ntiles < 65536 ? ntiles : 65536); }

template <int C>
int launch_resample(void* out, float* y, const void* x, int B, int H, int W, int H2, int W2, const int* h_lo, const int* h_kk, int hk,
                    const int* v_lo, const int* v_kk, int vk, hipStream_t stream) {
    const int tyn = (int)ideas_cdiv(H2, TH), txn = (int)ideas_cdiv(W2, TW);
    const int64_t ntiles = (int64_t)B * tyn * txn;
    // four bytes a store: every output row starts on a 4-byte boundary and ends on one
    const bool vec = ((int64_t)W2 * C) % 4 == 0 && ideas_aligned<4>(out) && ideas_aligned16(y);
    const bool vin = ((int64_t)W * C) % 4 == 0 && ideas_aligned<4>(x);      // every input row starts on a word
    if (vec)
        hipLaunchKernelGGL((resample_kernel<C, true>), dim3(tile_grid(ntiles)), dim3(256), 0, stream, (unsigned char*)out, y,
                           (const unsigned char*)x, H, W, H2, W2, h_lo, h_kk, hk, v_lo, v_kk, vk, tyn, txn, ntiles, vin);
    else
        hipLaunchKernelGGL((resample_kernel<C, false>), dim3(tile_grid(ntiles)), dim3(256), 0, stream, (unsigned char*)out, y,
                           (const unsigned char*)x, H, W, H2, W2, h_lo, h_kk, hk, v_lo, v_kk, vk, tyn, txn, ntiles, vin);
    return ideas_launch_status();
}

// ---- median -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void sort2(unsigned& a, unsigned& b) {
    const unsigned lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
}

// the median of 9 in 19 exchanges (the network of Paeth / Smith; N. Devillard, "Fast median search", 1998)
__device__ __forceinline__ unsigned median9(unsigned (&p)[9]) {
    sort2(p[1], p[2]); sort2(p[4], p[5]); sort2(p[7], p[8]);
    sort2(p[0], p[1]); sort2(p[3], p[4]); sort2(p[6], p[7]);
    sort2(p[1], p[2]); sort2(p[4], p[5]); sort2(p[7], p[8]);
    sort2(p[0], p[3]); sort2(p[5], p[8]); sort2(p[4], p[7]);
    sort2(p[3], p[6]); sort2(p[1], p[4]); sort2(p[2], p[5]);
    sort2(p[4], p[7]); sort2(p[4], p[2]); sort2(p[6], p[4]);
    sort2(p[4], p[2]);
    return p[4];
}

// The median of N = 2 m + 1 values by forgetful selection: of any m + 2 of them neither the smallest nor the largest can be the median
// (m + 1 others lie on one side of it).  Keep m + 2 values, move their minimum to the front and their maximum to the back by
// exchanges, forget both, take one value not yet seen into the freed slot, and repeat one shorter, until one value is left.  Every
// index is a constant once the loops are unrolled: N = 25 is 12 rounds over 14, 13, ... 3 values, 132 exchanges.
template <int N>
__device__ __forceinline__ unsigned median_select(unsigned (&a)[N]) {
    constexpr int M = N / 2;
    int next = M + 2;
#pragma unroll
    for (int s = 0; s < M; ++s) {
        const int cnt = M + 2 - s, last = s + cnt - 1;       // the live values: a[s .. last]
#pragma unroll
        for (int k = 0; k < cnt / 2; ++k) sort2(a[s + k], a[last - k]);          // pairs: the smaller to the front half
#pragma unroll
        for (int k = 1; k < (cnt + 1) / 2; ++k) sort2(a[s], a[s + k]);           // minimum of the front half (and the middle)
#pragma unroll
        for (int k = cnt / 2; k < cnt - 1; ++k) sort2(a[s + k], a[last]);        // maximum of the back half (and the middle)
        if (next < N) a[last] = a[next++];                   // (the last round, over three values, has none left to take)
    }
    return a[M];
}

// A workgroup owns MTH x TW output pixels and stages them with their halo, edge-replicated, in LDS: rows of words that begin HB bytes
// (the halo's R * C bytes rounded up to a word) before the tile's first byte.  A thread's four output bytes at byte 4 d of the tile
// have their K windows in bytes 4 d + OFF0 .. 4 d + OFF0 + 2 R C + 3 of the staged row: NW words from word d, every byte of which is
// picked by a compile-time index.  VEC also loads the words that lie wholly inside the image row as words.
template <int C, int K, bool VEC>
__global__ __launch_bounds__(256) void median_kernel(unsigned char* __restrict__ out, float* __restrict__ y,
                                                     const unsigned char* __restrict__ x, int H, int W, int tyn, int txn, int64_t ntiles) {
    constexpr int R = K / 2, TWD = TW * C / 4, HB = (R * C + 3) / 4 * 4, OFF0 = HB - R * C, NW = (OFF0 + 2 * R * C + 4 + 3) / 4;
    constexpr int PD = TWD + NW - 1, SR = MTH + K - 1;
    __shared__ unsigned s_t[SR * PD];
    __shared__ float s_unit[256];
    const int tid = threadIdx.x;
    fill_unit(s_unit);
    const int64_t rowb = (int64_t)W * C;

    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int tx = (int)(tile % txn), ty = (int)((tile / txn) % tyn);
        const int64_t b = tile / txn / tyn;
        const int ox0 = tx * TW, oy0 = ty * MTH;
        const int tw = W - ox0 < TW ? W - ox0 : TW, th = H - oy0 < MTH ? H - oy0 : MTH;
        const unsigned char* xb = x + b * H * rowb;
        __syncthreads();
        for (int i = tid; i < SR * PD; i += 256) {
            const int sy = i / PD, sd = i % PD;
            const unsigned char* xr = xb + clampi(oy0 + sy - R, 0, H - 1) * rowb;
            const int64_t n = (int64_t)ox0 * C - HB + 4 * sd;                     // the word's first byte in the image row
            unsigned w = 0;
            if (VEC && n >= 0 && n + 4 <= rowb) {
                w = *reinterpret_cast<const unsigned*>(xr + n);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int64_t m = n + e + 8 * C;                             // (>= 0: HB <= 8 C)
                    const int64_t px = m / C - 8;
                    const int pc = px < 0 ? 0 : (px > W - 1 ? W - 1 : (int)px);  // replicated first and last column
                    w |= (unsigned)xr[(int64_t)pc * C + (int)(m % C)] << (8 * e);
                }
            }
            s_t[i] = w;
        }
        __syncthreads();
        for (int i = tid; i < th * TWD; i += 256) {
            const int orow = i / TWD, d = i % TWD;
            const int nvalid = tw * C - 4 * d;
            if (nvalid <= 0) continue;
            unsigned w[K][NW];
#pragma unroll
            for (int dy = 0; dy < K; ++dy)
#pragma unroll
                for (int k = 0; k < NW; ++k) w[dy][k] = s_t[(orow + dy) * PD + d + k];
            unsigned ob[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned v[K * K];
#pragma unroll
                for (int dy = 0; dy < K; ++dy)
#pragma unroll
                    for (int dx = 0; dx < K; ++dx) v[dy * K + dx] = byte_of(w[dy], OFF0 + dx * C + e);
                if constexpr (K == 3) ob[e] = median9(v);
                else ob[e] = median_select(v);
            }
            const int64_t o = ((b * H + oy0 + orow) * W + ox0) * C + 4 * d;
            store_bytes<4, VEC ? 4 : 0>(out, y, o, ob, nvalid, unit_table{s_unit});    // VEC: nvalid is 4 in every word
        }
    }
}

template <int C, int K>
int launch_median(void* out, float* y, const void* x, int B, int H, int W, hipStream_t stream) {
    const int tyn = (int)ideas_cdiv(H, MTH), txn = (int)ideas_cdiv(W, TW);
    const int64_t ntiles = (int64_t)B * tyn * txn;
    const bool vec = ((int64_t)W * C) % 4 == 0 && ideas_aligned<4>(out) && ideas_aligned<4>(x) && ideas_aligned16(y);
    if (vec)
        hipLaunchKernelGGL((median_kernel<C, K, true>), dim3(tile_grid(ntiles)), dim3(256), 0, stream, (unsigned char*)out, y,
                           (const unsigned char*)x, H, W, tyn, txn, ntiles);
    else
        hipLaunchKernelGGL((median_kernel<C, K, false>), dim3(tile_grid(ntiles)), dim3(256), 0, stream, (unsigned char*)out, y,
                           (const unsigned char*)x, H, W, tyn, txn, ntiles);
    return ideas_launch_status();
}

}  // namespace

extern "C" int ideas_resample_u8(void* out_u8, void* y, const void* x_u8, int B, int C, int H, int W, int H2, int W2,
                                 const int32_t* h_lo, const int32_t* h_kk, int h_ksize, const int32_t* v_lo, const int32_t* v_kk,
                                 int v_ksize, void* stream_) {
    if (!x_u8 || !out_u8) return IDEAS_E_NULL;
    if ((h_lo == nullptr) != (h_kk == nullptr) || (v_lo == nullptr) != (v_kk == nullptr)) return IDEAS_E_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || H2 <= 0 || W2 <= 0 || (C != 1 && C != 3)) return IDEAS_E_SHAPE;
    if ((!h_lo && W2 != W) || (!v_lo && H2 != H)) return IDEAS_E_SHAPE;
    if (h_lo && (h_ksize < 1 || h_ksize > KMAX)) return IDEAS_E_UNSUPPORTED;
    if (v_lo && (v_ksize < 1 || v_ksize > KMAX)) return IDEAS_E_UNSUPPORTED;
    const int hk = h_lo ? h_ksize : 1, vk = v_lo ? v_ksize : 1;
    hipStream_t stream = (hipStream_t)stream_;
    return C == 3 ? launch_resample<3>(out_u8, (float*)y, x_u8, B, H, W, H2, W2, h_lo, h_kk, hk, v_lo, v_kk, vk, stream)
                  : launch_resample<1>(out_u8, (float*)y, x_u8, B, H, W, H2, W2, h_lo, h_kk, hk, v_lo, v_kk, vk, stream);
}

extern "C" int ideas_median_u8(void* out_u8, void* y, const void* x_u8, int B, int C, int H, int W, int K, void* stream_) {
    if (!x_u8 || !out_u8) return IDEAS_E_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || (C != 1 && C != 3)) return IDEAS_E_SHAPE;
    if (K != 3 && K != 5) return IDEAS_E_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    float* yf = (float*)y;
    if (C == 3) return K == 3 ? launch_median<3, 3>(out_u8, yf, x_u8, B, H, W, stream) : launch_median<3, 5>(out_u8, yf, x_u8, B, H, W, stream);
    return K == 3 ? launch_median<1, 3>(out_u8, yf, x_u8, B, H, W, stream) : launch_median<1, 5>(out_u8, yf, x_u8, B, H, W, stream);
}
