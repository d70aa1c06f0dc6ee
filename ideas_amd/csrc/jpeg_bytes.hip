// The JPEG FILE, written on the device: from the quantised coefficients of ideas_jpeg_file_roundtrip (attack_jpeg.hip) to the bytes
// libjpeg / libjpeg-turbo writes with its defaults -- header, Huffman coding with the Annex K tables, bit packing, byte stuffing.  The
// stream is stated in include/ideas_hip.h ("The JPEG file, written") and restated in Python by tests/jpegbytes_ref.py, which
// tests/test_jpeg_bytes.py holds to Pillow's own files.  jpeg_block.hpp gives the quantiser tables and jpeg_scan.hpp the walk over
// the scan, shared with the reader (jpeg_decode.hip); nothing else of the round trip is used here.
//
// A block's code has a variable length, so the file is made in four launches behind one memset:
//   code_kernel<false>   one thread a block of the scan, in scan order: the number of bits of its code.  The DC predictor and the dummy
//                        luma blocks of 4:2:0 are index arithmetic on the coefficient arrays, so no thread waits for another.
//   scan_kernel          one workgroup an image: the exclusive prefix sum of those counts, 64-bit, in place, 1024 blocks a trip.
//   code_kernel<true>    the same walk again, this time writing the bits at the block's offset into a cleared buffer of 32-bit words,
//                        kept in stream order (most significant bit first, the word stored byte-swapped).  A block's first and last
//                        word are shared with its neighbours and go out by atomicOr, the words between by plain stores.
//   stuff_kernel         one workgroup an image: header, then the scan 4096 bytes a trip -- pad the last byte with ones, count the FF
//                        bytes a thread, prefix sum, lay the bytes with their 00s out in LDS, copy the tile to the file -- then FFD9 and
//                        the length.
// Both walks are ONE function (code_block) with two sinks, so the counts and the bits cannot disagree.  A coefficient without a code
// is coded as the largest category instead and flags its image: the sizes stay inside the bound, and the image's length becomes -1.
// DESIGN.md 3.15.1.
#include <initializer_list>
#include "jpeg_block.hpp"
#include "jpeg_scan.hpp"

namespace {

// ISO/IEC 10918-1 Annex K.3 - K.6: the number of codes of each length 1..16 and the symbols in order of their codes
struct huff_spec {
    unsigned char bits[16];
    unsigned char vals[162];
    int n;
};
constexpr huff_spec K_DC_LUMA = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr huff_spec K_DC_CHROMA = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr huff_spec K_AC_LUMA = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    162};
constexpr huff_spec K_AC_CHROMA = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    162};

// symbol -> code | length << 16: the canonical codes of Annex C (lengths ascending, codes counting up), made by the compiler
struct huff_lut {
    unsigned v[256];
};
constexpr huff_lut make_lut(const huff_spec& s) {
    huff_lut t = {};
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < s.bits[len - 1]; ++i) t.v[s.vals[k++]] = code++ | ((unsigned)len << 16);
        code <<= 1;
    }
    return t;
}
// DC0, AC0, DC1, AC1: the order of the header's DHT segments
__device__ const huff_lut k_lut[4] = {make_lut(K_DC_LUMA), make_lut(K_AC_LUMA), make_lut(K_DC_CHROMA), make_lut(K_AC_CHROMA)};

// The header with C = 1 ([0]: 328 bytes) and C = 3 ([1]: 623 bytes), made by the compiler: everything but the 64 bytes of each DQT,
// H, W and the luma sampling factors, which header_byte fills in.
constexpr int HDR_1 = 328, HDR_3 = 623, HDR_DQT = 25, HDR_DQT_STEP = 69;
struct header_bytes {
    unsigned char v[2][HDR_3 + 1];
};
constexpr void put(unsigned char* v, int& n, std::initializer_list<int> bytes) {
    for (int b : bytes) v[n++] = (unsigned char)b;
}
constexpr void put_dht(unsigned char* v, int& n, const huff_spec& s, int id) {
    put(v, n, {0xff, 0xc4, 0x00, 19 + s.n, id});
    for (int i = 0; i < 16; ++i) v[n++] = s.bits[i];
    for (int i = 0; i < s.n; ++i) v[n++] = s.vals[i];
}
constexpr header_bytes make_headers() {
    header_bytes h = {};
    for (int k = 0; k < 2; ++k) {
        const int C = k ? 3 : 1;
        unsigned char* v = h.v[k];
        int n = 0;
        put(v, n, {0xff, 0xd8, 0xff, 0xe0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
        for (int i = 0; i < (k ? 2 : 1); ++i) {
            put(v, n, {0xff, 0xdb, 0x00, 0x43, i});
            n += 64;
        }
        put(v, n, {0xff, 0xc0, 0x00, 8 + 3 * C, 8, 0, 0, 0, 0, C, 1, 0x11, 0});
        if (k) put(v, n, {2, 0x11, 1, 3, 0x11, 1});
        put_dht(v, n, K_DC_LUMA, 0x00);
        put_dht(v, n, K_AC_LUMA, 0x10);
        if (k) {
            put_dht(v, n, K_DC_CHROMA, 0x01);
            put_dht(v, n, K_AC_CHROMA, 0x11);
        }
        put(v, n, {0xff, 0xda, 0x00, 6 + 2 * C, C, 1, 0x00});
        if (k) put(v, n, {2, 0x11, 3, 0x11});
        put(v, n, {0x00, 0x3f, 0x00});
        v[HDR_3] = (unsigned char)(n == (k ? HDR_3 : HDR_1));          // checked below
    }
    return h;
}
constexpr header_bytes K_HEADERS = make_headers();
static_assert(K_HEADERS.v[0][HDR_3] == 1 && K_HEADERS.v[1][HDR_3] == 1, "the headers are 328 and 623 bytes");
__device__ const header_bytes k_headers = K_HEADERS;

// byte i of the header of a C x H x W image at this quality and subsampling
__device__ __forceinline__ unsigned header_byte(int i, int C, int H, int W, int sub, int qscale) {
    const int sof = HDR_DQT - 5 + HDR_DQT_STEP * (C == 3 ? 2 : 1);       // the SOF0 marker
    unsigned v = k_headers.v[C == 3][i];
    if (i >= HDR_DQT && i < sof) {
        const int t = (i - HDR_DQT) / HDR_DQT_STEP, j = (i - HDR_DQT) % HDR_DQT_STEP;
        if (j < 64) v = (unsigned)jpeg_table_entry(t * 64 + k_zigzag[j], qscale);
    } else if (i == sof + 5) {
        v = (unsigned)H >> 8;
    } else if (i == sof + 6) {
        v = (unsigned)H & 255u;
    } else if (i == sof + 7) {
        v = (unsigned)W >> 8;
    } else if (i == sof + 8) {
        v = (unsigned)W & 255u;
    } else if (i == sof + 11) {
        v = C == 3 && sub == 2 ? 0x22u : 0x11u;
    }
    return v;
}

// the number of bits of |v|: the category of a DC difference or an AC coefficient
__device__ __forceinline__ int category(int v) { return 32 - __clz(v < 0 ? -v : v); }
// code and length of `lut`'s entry followed by the low nb bits of v (v >= 0) or of v - 1 (v < 0): at most 16 + 11 bits
template <class Sink> __device__ __forceinline__ void put_coded(Sink& sink, unsigned entry, int v, int nb) {
    const unsigned extra = (unsigned)(v + (v >> 31)) & ((1u << nb) - 1u);
    sink.put(((entry & 0xffffu) << nb) | extra, (int)(entry >> 16) + nb);
}

// One block: s its 64 coefficients at index 8 u + v, pred the DC of the component's previous block, dc / ac the component's tables
// (symbol -> code | length << 16).  Returns false where a coefficient had no code (and was coded as the largest category).
template <class Sink>
__device__ __forceinline__ bool code_block(Sink& sink, const short* s, int pred, const unsigned* dc, const unsigned* ac) {
    bool ok = true;
    const int d = (int)s[0] - pred;
    int nb = category(d);
    if (nb > 11) { ok = false; nb = 11; }
    put_coded(sink, dc[nb], d, nb);
    int r = 0;
    for (int k = 1; k < 64; ++k) {
        const int c = s[k_zigzag[k]];
        if (c == 0) {
            ++r;
            continue;
        }
        for (; r > 15; r -= 16) sink.put(ac[0xf0] & 0xffffu, (int)(ac[0xf0] >> 16));
        nb = category(c);
        if (nb > 10) { ok = false; nb = 10; }
        put_coded(sink, ac[(r << 4) | nb], c, nb);
        r = 0;
    }
    if (r > 0) sink.put(ac[0] & 0xffffu, (int)(ac[0] >> 16));
    return ok;
}

struct bit_counter {
    unsigned n = 0;
    __device__ __forceinline__ void put(unsigned, int nbits) { n += (unsigned)nbits; }
};

// Bits from bit offset `off` of a cleared buffer of words in stream order.  acc holds `fill` < 32 pending bits behind the zeros that
// stand for the bits in front of `off` in the first word; that word and the last one go out by atomicOr.
struct bit_writer {
    unsigned* w;
    uint64_t acc = 0;
    int fill;
    bool shared;
    __device__ __forceinline__ bit_writer(unsigned* words, uint64_t off) : w(words + (off >> 5)), fill((int)(off & 31u)), shared(fill != 0) {}
    __device__ __forceinline__ void put(unsigned v, int nbits) {                   // nbits <= 27
        acc = (acc << nbits) | v;
        fill += nbits;
        if (fill >= 32) {
            fill -= 32;
            const unsigned word = __builtin_bswap32((unsigned)(acc >> fill));
            if (shared) atomicOr(w, word); else *w = word;
            shared = false;
            ++w;
        }
    }
    __device__ __forceinline__ void finish() {
        if (fill > 0) atomicOr(w, __builtin_bswap32((unsigned)(acc << (32 - fill))));
    }
};

constexpr int BLK_LD = 33;         // words from one thread's block to the next in LDS: a wave's reads of one coefficient fall on all banks

// One thread a block of the scan.  EMIT false: offs[image][block] = the bits of its code, bad[image] |= 1 where a coefficient has no
// code.  EMIT true: offs holds the exclusive prefix sums; the bits go to raw + image * raw_words.
template <bool EMIT>
__global__ __launch_bounds__(256) void code_kernel(uint64_t* __restrict__ offs, unsigned* __restrict__ raw, int* __restrict__ bad,
                                                   const short* __restrict__ coef_y, const short* __restrict__ coef_c, scan_geom g,
                                                   int64_t raw_words, int64_t total) {
    __shared__ unsigned s_blk[256 * BLK_LD];
    __shared__ unsigned s_dc[2][16], s_ac[2][256];
    for (int i = threadIdx.x; i < 512; i += 256) s_ac[i >> 8][i & 255] = k_lut[(i >> 8) * 2 + 1].v[i & 255];
    if (threadIdx.x < 32) s_dc[threadIdx.x >> 4][threadIdx.x & 15] = k_lut[(threadIdx.x >> 4) * 2].v[threadIdx.x & 15];
    __syncthreads();
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gi >= total) return;
    const int64_t b = gi / g.nblk, k = gi - b * g.nblk;
    const int64_t mcu = k / g.per_mcu;
    const int slot = (int)(k - mcu * g.per_mcu), nluma = g.hs * g.hs;
    const bool chroma = slot >= nluma;

    // the block's coefficients (null: a dummy), its DC and its predictor
    const short* src;
    int dcv, pred = 0;
    if (chroma) {
        const short* plane = coef_c + (b * 2 + (slot - nluma)) * g.nmcu * 64;
        src = plane + mcu * 64;
        dcv = src[0];
        if (mcu > 0) pred = src[-64];
    } else {
        const short* plane = coef_y + b * g.bhn * g.bwn * 64;
        const int my = (int)(mcu / g.mw), mx = (int)(mcu - (int64_t)my * g.mw);
        int by, bx;
        const bool real = luma_source(g, my, mx, slot, by, bx);
        src = plane + ((int64_t)by * g.bwn + bx) * 64;
        dcv = src[0];
        if (!real) src = nullptr;
        if (slot > 0 || mcu > 0) {                           // the luma block before this one in the scan
            const int64_t pm = slot > 0 ? mcu : mcu - 1;
            const int pmy = (int)(pm / g.mw), pmx = (int)(pm - (int64_t)pmy * g.mw);
            luma_source(g, pmy, pmx, slot > 0 ? slot - 1 : nluma - 1, by, bx);
            pred = plane[((int64_t)by * g.bwn + bx) * 64];
        }
    }

    unsigned* row = s_blk + threadIdx.x * BLK_LD;            // this thread's own: no barrier
    if (!src) {
        row[0] = (unsigned)dcv & 0xffffu;
#pragma unroll
        for (int i = 1; i < 32; ++i) row[i] = 0;
    } else if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint4 v = reinterpret_cast<const uint4*>(src)[i];
            row[4 * i] = v.x; row[4 * i + 1] = v.y; row[4 * i + 2] = v.z; row[4 * i + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 32; ++i) row[i] = ((unsigned)src[2 * i] & 0xffffu) | ((unsigned)src[2 * i + 1] << 16);
    }
    const short* s = reinterpret_cast<const short*>(row);

    if constexpr (EMIT) {
        bit_writer sink(raw + b * raw_words, offs[gi]);
        code_block(sink, s, pred, s_dc[chroma], s_ac[chroma]);
        sink.finish();
    } else {
        bit_counter sink;
        if (!code_block(sink, s, pred, s_dc[chroma], s_ac[chroma])) atomicOr(bad + b, 1);
        offs[gi] = sink.n;
    }
}

// offs[image][0 .. nblk): counts in, exclusive prefix sums out; bits[image] = their sum.  One workgroup an image, 4 blocks a thread a
// trip (at most 1024 * 1660 bits: 32 bits hold a trip's sum), the carry in 64 bits.
__global__ __launch_bounds__(256) void scan_kernel(uint64_t* __restrict__ offs, uint64_t* __restrict__ bits, int64_t nblk) {
    __shared__ unsigned s_w[4];
    uint64_t* p = offs + (int64_t)blockIdx.x * nblk;
    uint64_t carry = 0;
    for (int64_t base = 0; base < nblk; base += 1024) {
        const int64_t i0 = base + threadIdx.x * 4;
        unsigned v[4], sum = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = i0 + j < nblk ? (unsigned)p[i0 + j] : 0u;
            sum += v[j];
        }
        unsigned total;
        uint64_t at = carry + block_scan(sum, s_w, total);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i0 + j < nblk) p[i0 + j] = at;
            at += v[j];
        }
        carry += total;
    }
    if (threadIdx.x == 0) bits[blockIdx.x] = carry;
}

constexpr int STUFF_TILE = 4096;   // scan bytes a trip of stuff_kernel: 16 a thread

// One workgroup an image: the header, the scan bytes of raw (bits[image] bits, the last byte padded with ones) with a 00 behind every
// FF, FFD9, and nbytes[image] = the length, or -1 where bad[image] is set.
__global__ __launch_bounds__(256) void stuff_kernel(unsigned char* __restrict__ files, int* __restrict__ nbytes, int64_t row_stride,
                                                    const unsigned char* __restrict__ raw, int64_t raw_stride,
                                                    const uint64_t* __restrict__ bits, const int* __restrict__ bad, int C, int H, int W,
                                                    int sub, int qscale) {
    __shared__ unsigned s_w[4];
    __shared__ unsigned char s_out[2 * STUFF_TILE];
    unsigned char* out = files + (int64_t)blockIdx.x * row_stride;
    const unsigned char* in = raw + (int64_t)blockIdx.x * raw_stride;
    const int hdr = C == 3 ? HDR_3 : HDR_1;
    for (int i = threadIdx.x; i < hdr; i += 256) out[i] = (unsigned char)header_byte(i, C, H, W, sub, qscale);

    const uint64_t nbits = bits[blockIdx.x];
    const int64_t nraw = (int64_t)((nbits + 7) >> 3);
    const unsigned pad = (1u << (unsigned)((uint64_t)nraw * 8 - nbits)) - 1u;
    int64_t at = hdr;                                         // where the tile's first byte goes
    for (int64_t t0 = 0; t0 < nraw; t0 += STUFF_TILE) {
        const int64_t i0 = t0 + threadIdx.x * 16;
        const int n = (int)max((int64_t)0, min((int64_t)16, nraw - i0));      // this thread's bytes
        unsigned w[4] = {0, 0, 0, 0};
        if (n > 0) {
            const uint4 v = *reinterpret_cast<const uint4*>(in + i0);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        }
        unsigned by[16], ff = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            by[j] = byte_of(w, j) | (i0 + j == nraw - 1 ? pad : 0u);
            ff += (j < n && by[j] == 0xffu) ? 1u : 0u;
        }
        unsigned tile_ff;
        unsigned o = threadIdx.x * 16 + block_scan(ff, s_w, tile_ff);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (j < n) {
                s_out[o++] = (unsigned char)by[j];
                if (by[j] == 0xffu) s_out[o++] = 0;
            }
        }
        __syncthreads();
        const int tile_n = (int)min((int64_t)STUFF_TILE, nraw - t0) + (int)tile_ff;
        for (int j = threadIdx.x; j < tile_n; j += 256) out[at + j] = s_out[j];
        at += tile_n;                                         // (the next trip's block_scan has a barrier in front of its s_out stores)
    }
    if (threadIdx.x == 0) {
        out[at] = 0xff;
        out[at + 1] = 0xd9;
        nbytes[blockIdx.x] = bad[blockIdx.x] ? -1 : (int)(at + 2);
    }
}

// What a call needs, from its arguments; ok = false for arguments the encoder refuses (shape, subsampling, or a size beyond an int
// of bytes a file or of blocks a launch).  B <= 0 plans one image.
struct enc_plan {
    bool ok = false;
    scan_geom g;
    int hdr;
    int64_t max_bytes;             // header + 416 a block + 3
    int64_t raw_stride;            // bytes of one image's unstuffed scan: 208 a block and a word to spare, a multiple of 16
    size_t offs_bytes, cleared_at, raw_at, bytes;        // the workspace behind its 16-byte alignment: offs, bits | bad, raw (cleared)
};

enc_plan plan_for(int B, int C, int H, int W, int sub) {
    enc_plan p;
    if ((C != 1 && C != 3) || H <= 0 || W <= 0 || H > 65535 || W > 65535 || (sub != 0 && sub != 2)) return p;
    p.g = make_scan_geom(C, H, W, sub);
    const scan_geom& g = p.g;
    p.hdr = C == 3 ? HDR_3 : HDR_1;
    p.max_bytes = p.hdr + 416 * g.nblk + 3;
    const int64_t nb = B > 0 ? B : 1;
    if (p.max_bytes > INT32_MAX || nb * g.nblk > INT32_MAX) return p;
    p.raw_stride = (208 * g.nblk + 4 + 15) / 16 * 16;
    p.offs_bytes = (size_t)nb * (size_t)g.nblk * 8;
    p.cleared_at = p.offs_bytes + (size_t)nb * 8;
    p.raw_at = (p.cleared_at + (size_t)nb * 4 + 15) / 16 * 16;
    p.bytes = p.raw_at + (size_t)nb * (size_t)p.raw_stride + 16;          // 16: the alignment of a workspace that arrives unaligned
    p.ok = true;
    return p;
}

}  // namespace

extern "C" size_t ideas_jpeg_file_max_bytes(int C, int H, int W, int subsampling) {
    const enc_plan p = plan_for(1, C, H, W, subsampling);
    return p.ok ? (size_t)p.max_bytes : 0;
}

extern "C" size_t ideas_jpeg_file_encode_workspace_bytes(int B, int C, int H, int W, int subsampling) {
    if (B <= 0) return 0;
    const enc_plan p = plan_for(B, C, H, W, subsampling);
    return p.ok ? p.bytes : 0;
}

extern "C" int ideas_jpeg_file_encode(void* files, int* nbytes, long long row_stride, const short* coef_y, const short* coef_c,
                                      void* workspace, int B, int C, int H, int W, int quality, int subsampling, void* stream_) {
    if (!files || !nbytes || !coef_y || !workspace || (C == 3 && !coef_c)) return IDEAS_E_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || H > 65535 || W > 65535 || (C != 1 && C != 3)) return IDEAS_E_SHAPE;
    if (quality < 1 || quality > 100) return IDEAS_E_UNSUPPORTED;
    if (subsampling != 0 && subsampling != 2) return IDEAS_E_UNSUPPORTED;
    const enc_plan p = plan_for(B, C, H, W, subsampling);
    if (!p.ok || row_stride < p.max_bytes) return IDEAS_E_SHAPE;
    hipStream_t stream = (hipStream_t)stream_;

    unsigned char* base = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(workspace) + 15) & ~(uintptr_t)15);
    uint64_t* offs = reinterpret_cast<uint64_t*>(base);
    uint64_t* bits = reinterpret_cast<uint64_t*>(base + p.offs_bytes);
    int* bad = reinterpret_cast<int*>(base + p.cleared_at);
    unsigned char* raw = base + p.raw_at;
    // the flags and the words the bits are ORed into, in one stretch
    const hipError_t e = hipMemsetAsync(bad, 0, p.raw_at - p.cleared_at + (size_t)B * (size_t)p.raw_stride, stream);
    if (e != hipSuccess) return (int)e;

    const int64_t total = (int64_t)B * p.g.nblk;
    const dim3 grid((unsigned)ideas_cdiv(total, 256));
    const int64_t raw_words = p.raw_stride / 4;
    hipLaunchKernelGGL((code_kernel<false>), grid, dim3(256), 0, stream, offs, (unsigned*)raw, bad, coef_y, coef_c, p.g, raw_words, total);
    hipLaunchKernelGGL(scan_kernel, dim3(B), dim3(256), 0, stream, offs, bits, p.g.nblk);
    hipLaunchKernelGGL((code_kernel<true>), grid, dim3(256), 0, stream, offs, (unsigned*)raw, bad, coef_y, coef_c, p.g, raw_words, total);
    hipLaunchKernelGGL(stuff_kernel, dim3(B), dim3(256), 0, stream, (unsigned char*)files, nbytes, (int64_t)row_stride,
                       (const unsigned char*)raw, p.raw_stride, bits, bad, C, H, W, subsampling, jpeg_qscale(quality));
    return ideas_launch_status();
}
