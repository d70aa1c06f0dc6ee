// The JPEG FILE, read on the device: from the entropy-coded segment of a baseline file (behind the SOS header, still stuffed) to the
// quantised coefficients and the pixels libjpeg / libjpeg-turbo decodes from it -- Pillow's Image.open, to the byte.  The contract is
// stated in include/ideas_hip.h ("The JPEG file, read") and restated in Python by tests/jpegdecode_ref.py, which tests/test_jpeg_decode.py
// holds to Pillow's own pixels.  jpeg_scan.hpp gives the walk over the scan (shared with the writer, jpeg_bytes.hip), jpeg_islow.hpp the
// inverse transform and the upsampler (shared with the round trip, attack_jpeg.hip).
//
// A Huffman stream cannot be cut at known places, so the block boundaries are FOUND in parallel.  Behind the memsets:
//   unstuff_kernel     one workgroup an image, the inverse of stuff_kernel: drop the 00 behind every FF, stop at the first FF xx with
//                      xx != 00, prefix sum, compact the clean bytes into the workspace, 16 bytes of FF behind them (bits read past the
//                      end count as 1), the clean bit length and the number of subsequences to the workspace.
//   sync_kernel        one workgroup an image.  The clean stream is cut into subsequences of L = IDEAS_JPEG_SUBSEQ_BITS bits.  The
//                      decoder's state between two symbols is (bit position p, slot of the block in its MCU, zigzag index z); f_i(state)
//                      decodes symbols from `state` until p reaches the end of subsequence i and returns the state there and the number
//                      of blocks finished.  The true states solve in_0 = (0, 0, 0), in_i = out_{i-1}, out_i = f_i(in_i).  Every in_i
//                      (i > 0) starts at the guess (i L, 0, 0); a round re-decodes the subsequences whose input changed, a barrier,
//                      the outputs are handed on, until nothing changed.  After round r subsequences 0..r are exact, so nsub + 1 rounds
//                      are the loop's hard limit; the fixed point is unique, so scheduling cannot change the result.  Then the prefix
//                      sum of the block counts: the scan-order index of the first block of each subsequence.
//   emit_kernel        one thread a subsequence, over the batch (a workgroup: 256 subsequences of one image): decode once more from the
//                      converged state, the non-zero AC values
//                      through the zigzag table into the (cleared) coefficient arrays, the DC DIFFERENCE of each block into an int32
//                      array in scan order.  A block that straddles a boundary is written by both owners, each its own coefficients.
//   dc_kernel          one workgroup an image and component: the prefix sum of the differences in scan order, dummies included, to
//                      coef[..][0], range-checked.
//   pixel kernels      dequantise, the two idct_pass, clamp, the 4:2:0 upsampler, colour out, store8 -- the lane mapping of the round
//                      trip.  4:2:0 takes two launches through the half-resolution planes in the workspace, as there.
// Both decoding kernels run ONE function (decode_span) with two sinks, so the boundaries found and the coefficients written cannot
// disagree.  Every symbol consumes at least one bit and at most 27 (a bit pattern without a code consumes 16), so decode_span's loop
// is bounded by L + 27 bits whatever the bytes are.  Both read the stream out of LDS: a workgroup stages the words of its 256
// subsequences (stage_window).  Every store is addressed by the block's index in the scan, which is checked against
// the scan's block count, never by the data.  status[] is the corrupt flag itself: cleared by a memset, raised by atomicOr.
// This file is compiled with -fwrapv (Makefile): the transform of coefficients no encoder produces may wrap, and wrapping is defined.
// DESIGN.md 3.15.1.
#include <algorithm>
#include "jpeg_islow.hpp"
#include "jpeg_scan.hpp"

namespace {

constexpr int L = IDEAS_JPEG_SUBSEQ_BITS;
constexpr unsigned DIRTY = 0x80000000u;            // bit 31 of a state's second word: its subsequence has to be decoded again

// ------------------------------------------------------------------------------------------------ the Huffman tables, in LDS
// One table of a DHT segment (16 counts, then the symbols in order of their codes) as the decoder wants it: lut[first 8 bits] =
// length << 8 | symbol for the codes of at most 8 bits (0: longer, or none); for the lengths 9..16 the largest code of that length
// (-1: none) and what to add to a code to get its symbol's index.
struct huff_dec {
    unsigned short lut[256];
    int maxcode[17], off[17];
    unsigned char vals[256];
};

// s_tab[2 c + (0: DC, 1: AC)] from huff [C][2][16 + 256], by the whole workgroup (two barriers).  Counts that describe no prefix code
// give a table that decodes something; every index stays inside the table.
__device__ __forceinline__ void build_tables(huff_dec* s_tab, const unsigned char* __restrict__ huff, int C) {
    for (int i = threadIdx.x; i < 2 * C * 256; i += blockDim.x) {
        s_tab[i >> 8].lut[i & 255] = 0;
        s_tab[i >> 8].vals[i & 255] = huff[(i >> 8) * 272 + 16 + (i & 255)];
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * C) {
        huff_dec& t = s_tab[threadIdx.x];
        const unsigned char* counts = huff + threadIdx.x * 272;
        unsigned code = 0, k = 0;
        for (int len = 1; len <= 16; ++len) {
            const unsigned n = counts[len - 1];
            t.off[len] = (int)k - (int)code;
            for (unsigned i = 0; i < n; ++i, ++code, ++k) {
                if (len <= 8) {
                    const unsigned first = code << (8 - len);
                    for (unsigned j = 0; j < (1u << (8 - len)); ++j)
                        if (first + j < 256u) t.lut[first + j] = (unsigned short)((len << 8) | t.vals[k & 255u]);
                }
            }
            t.maxcode[len] = n ? (int)code - 1 : -1;
            code <<= 1;
        }
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------ the decoder
// The window: the words of 256 consecutive subsequences of one image and two more (a symbol that starts in the last one ends there),
// staged in LDS by the workgroup, because a thread's loads depend on each other symbol by symbol.  (Measured on 32 files of 256 x 256:
// 464 against 471 us for sync_kernel, 213 against 239 us for emit_kernel with the two words read from global memory at every symbol --
// the kernels wait for their own instructions)  A thread reads its own subsequence, WPS words on from its
// neighbour's: one word of padding a subsequence spreads the lanes over the banks.
constexpr int WPS = L / 32;                        // words a subsequence
constexpr int WIN_WORDS = 256 * WPS + 2;
constexpr int WIN_LDS = WIN_WORDS + WIN_WORDS / WPS + 1;
static_assert(L % 32 == 0 && (WPS & (WPS - 1)) == 0, "a subsequence is a power of two of words");
__device__ __forceinline__ int win_at(unsigned k) { return (int)(k + k / WPS); }

// s_win = the words w0 .. w0 + WIN_WORDS - 1 of `words`; behind nwords (the row's allocation): ones.  One barrier, behind the stores.
__device__ __forceinline__ void stage_window(unsigned* s_win, const unsigned* __restrict__ words, unsigned w0, unsigned nwords) {
    for (unsigned k = threadIdx.x; k < (unsigned)WIN_WORDS; k += 256) s_win[win_at(k)] = w0 + k < nwords ? words[w0 + k] : 0xffffffffu;
    __syncthreads();
}

// 32 bits of the clean stream from bit q of the window on, most significant first.  Reads the two words round q: up to 8 bytes behind
// the stream's last byte, where unstuff_kernel put FF.
__device__ __forceinline__ unsigned peek32(const unsigned* s_win, unsigned q) {
    const unsigned i = q >> 5;
    const uint64_t v = ((uint64_t)__builtin_bswap32(s_win[win_at(i)]) << 32) | __builtin_bswap32(s_win[win_at(i + 1)]);
    return (unsigned)(v >> (32 - (q & 31u)));
}

struct dec_state {
    unsigned p;                    // bit position
    int slot, z;                   // the block's place in its MCU; the next zigzag index (0: the DC comes next)
};
__device__ __forceinline__ uint2 pack_state(const dec_state& s) { return make_uint2(s.p, (unsigned)(s.slot << 6 | s.z)); }
__device__ __forceinline__ dec_state unpack_state(uint2 v) { return dec_state{v.x, (int)(v.y >> 6) & 7, (int)v.y & 63}; }

// Symbols from state s until s.p reaches `end` (<= the stream's bit length, and inside the window that starts at bit `base`); returns
// the number of blocks finished.  The sink sees
// dc(difference), ac(zigzag index, value), error() and block_done().  A symbol in error -- no code (16 bits consumed), a category
// above 11 (DC) or 10 (AC), a run past coefficient 63 -- ends its block; a symbol 0x10..0xE0 is an end of block, as in the library.
template <class Sink>
__device__ __forceinline__ unsigned decode_span(const unsigned* s_win, unsigned base, unsigned end, dec_state& s, const huff_dec* s_tab,
                                                int nluma, int per_mcu, Sink& sink) {
    unsigned done = 0;
    while (s.p < end) {
        const int comp = s.slot < nluma ? 0 : s.slot - nluma + 1;
        const huff_dec& t = s_tab[2 * comp + (s.z > 0)];
        const unsigned bits = peek32(s_win, s.p - base);
        const unsigned e = t.lut[bits >> 24];
        int len = (int)(e >> 8), sym = (int)(e & 255u);
        bool bad = false;
        if (len == 0) {
            for (len = 9; len <= 16; ++len) {
                const int code = (int)(bits >> (32 - len));
                if (code <= t.maxcode[len]) {
                    sym = t.vals[(code + t.off[len]) & 255];
                    break;
                }
            }
            if (len > 16) { len = 16; bad = true; }
        }
        const int nb = s.z == 0 ? sym : sym & 15, run = s.z == 0 ? 0 : sym >> 4;
        bad = bad || nb > (s.z == 0 ? 11 : 10);
        bool finished = false;
        if (bad) {
            s.p += (unsigned)len;
            sink.error();
            finished = true;
        } else {
            int v = 0;
            if (nb > 0) {
                const int extra = (int)((bits << len) >> (32 - nb));                 // len + nb <= 27
                v = extra < (1 << (nb - 1)) ? extra - (1 << nb) + 1 : extra;
            }
            s.p += (unsigned)(len + nb);
            if (s.z == 0) {
                sink.dc(v);
                s.z = 1;
            } else if (nb == 0) {
                if (run == 15) {                                                      // ZRL: a coefficient has to follow
                    s.z += 16;
                    if (s.z > 63) { sink.error(); finished = true; }
                } else {
                    finished = true;                                                  // EOB
                }
            } else {
                s.z += run;
                if (s.z > 63) {
                    sink.error();
                    finished = true;
                } else {
                    sink.ac(s.z, v);
                    finished = ++s.z == 64;
                }
            }
        }
        if (finished) {
            sink.block_done();
            ++done;
            s.z = 0;
            s.slot = s.slot + 1 == per_mcu ? 0 : s.slot + 1;
        }
    }
    return done;
}

struct null_sink {
    __device__ __forceinline__ void dc(int) {}
    __device__ __forceinline__ void ac(int, int) {}
    __device__ __forceinline__ void error() {}
    __device__ __forceinline__ void block_done() {}
};

// What emit_kernel does with the symbols of image b from block `blk` of the scan on.  Every address comes from blk < g.nblk.
struct emit_sink {
    const scan_geom& g;
    short* cy;                     // the image's luma blocks [bhn][bwn][64]
    short* cc;                     // its chroma blocks [2][nmcu][64]
    int* dcd;                      // its DC differences [nblk]
    int* status;                   // its flag
    int64_t blk;
    short* dst = nullptr;          // the coefficients of block blk; null: a dummy, or a block behind the scan
    __device__ __forceinline__ void set_block() {
        dst = nullptr;
        if (blk >= g.nblk) return;
        const int64_t mcu = blk / g.per_mcu;
        const int slot = (int)(blk - mcu * g.per_mcu), nluma = g.hs * g.hs;
        if (slot < nluma) {
            const int my = (int)(mcu / g.mw), mx = (int)(mcu - (int64_t)my * g.mw);
            int by, bx;
            if (luma_source(g, my, mx, slot, by, bx)) dst = cy + ((int64_t)by * g.bwn + bx) * 64;
        } else {
            dst = cc + ((slot - nluma) * g.nmcu + mcu) * 64;
        }
    }
    __device__ __forceinline__ void dc(int v) { if (blk < g.nblk) dcd[blk] = v; }
    __device__ __forceinline__ void ac(int z, int v) { if (dst) dst[k_zigzag[z]] = (short)v; }
    __device__ __forceinline__ void error() { if (blk < g.nblk) atomicOr(status, -1); }
    __device__ __forceinline__ void block_done() { ++blk; set_block(); }
};

// ------------------------------------------------------------------------------------------------ 1. unstuff
constexpr int UNSTUFF_TILE = 4096; // scan bytes a trip of unstuff_kernel: 16 a thread

// One workgroup an image.  scans row b, nbytes[b] bytes of it -> clean row b: the bytes in front of the first FF xx (xx != 00) without
// the 00 behind every FF, at most cap of them, and 16 bytes of FF; meta[2 b] = their bits, meta[2 b + 1] = the subsequences.
// nbytes[b] outside 0..row_stride flags the image; what is read stays inside its row.
__global__ __launch_bounds__(256) void unstuff_kernel(const unsigned char* __restrict__ scans, const int* __restrict__ nbytes,
                                                      int64_t row_stride, unsigned char* __restrict__ clean, int64_t clean_stride, int cap,
                                                      unsigned* __restrict__ meta, int* __restrict__ status) {
    __shared__ unsigned s_w[4];
    __shared__ int s_end;
    const unsigned char* in = scans + (int64_t)blockIdx.x * row_stride;
    unsigned char* out = clean + (int64_t)blockIdx.x * clean_stride;
    int n = nbytes[blockIdx.x];
    if (n < 0 || (int64_t)n > row_stride) {
        if (threadIdx.x == 0) atomicOr(status + blockIdx.x, -1);
        n = n < 0 ? 0 : (int)row_stride;
    }
    int64_t at = 0;                                          // clean bytes so far (the stores stop at cap)
    for (int64_t t0 = 0; t0 < n && at < cap; t0 += UNSTUFF_TILE) {
        if (threadIdx.x == 0) s_end = INT32_MAX;
        __syncthreads();
        const int64_t i0 = t0 + threadIdx.x * 16;
        unsigned by[18];                                     // the bytes i0 - 1 .. i0 + 16; outside the data: 00
#pragma unroll
        for (int j = 0; j < 18; ++j) {
            const int64_t a = i0 - 1 + j;
            by[j] = a >= 0 && a < n ? in[a] : 0u;
        }
        unsigned keep = 0;
        int first = INT32_MAX;                               // the first FF xx of this thread's bytes
#pragma unroll
        for (int j = 1; j <= 16; ++j) {
            const int64_t a = i0 + j - 1;
            if (a < n) {
                if (by[j] == 0xffu && a + 1 < n && by[j + 1] != 0u && first == INT32_MAX) first = (int)a;
                if (!(by[j] == 0u && by[j - 1] == 0xffu)) keep |= 1u << j;
            }
        }
        if (first != INT32_MAX) atomicMin(&s_end, first);
        __syncthreads();
        const int end = s_end;
        unsigned cnt = 0;
#pragma unroll
        for (int j = 1; j <= 16; ++j) cnt += ((keep >> j) & 1u) && i0 + j - 1 < end ? 1u : 0u;
        unsigned total;
        int64_t o = at + block_scan(cnt, s_w, total);
#pragma unroll
        for (int j = 1; j <= 16; ++j) {
            if (((keep >> j) & 1u) && i0 + j - 1 < end) {
                if (o < cap) out[o] = (unsigned char)by[j];
                ++o;
            }
        }
        at += total;
        if (end != INT32_MAX) break;                         // (uniform: s_end is read behind a barrier, and written behind the next)
    }
    if (at > cap) at = cap;
    if (threadIdx.x < 16) out[at + threadIdx.x] = 0xff;
    if (threadIdx.x == 0) {
        meta[2 * blockIdx.x] = (unsigned)at * 8u;
        meta[2 * blockIdx.x + 1] = (unsigned)((at * 8 + L - 1) / L);
    }
}

// ------------------------------------------------------------------------------------------------ 2. synchronise
// One workgroup an image; a thread owns the subsequences tid, tid + 256, ...  st_in / st_out: the states [B][nsub_max]; first: in the
// loop the blocks finished in each subsequence, at the end their exclusive prefix sum.  The three arrays carry values from thread to
// thread across the barriers, so they are not __restrict__.
__global__ __launch_bounds__(256) void sync_kernel(const unsigned char* __restrict__ clean, int64_t clean_stride,
                                                   const unsigned* __restrict__ meta, const unsigned char* __restrict__ huff,
                                                   uint2* st_in, uint2* st_out, unsigned* first, int* __restrict__ status,
                                                   int nsub_max, scan_geom g) {
    __shared__ huff_dec s_tab[6];
    __shared__ unsigned s_w[4];
    __shared__ unsigned s_win[WIN_LDS];
    build_tables(s_tab, huff, g.C);
    const unsigned* words = reinterpret_cast<const unsigned*>(clean + (int64_t)blockIdx.x * clean_stride);
    const unsigned nwords = (unsigned)(clean_stride / 4);
    const unsigned nbits = meta[2 * blockIdx.x], nsub = min(meta[2 * blockIdx.x + 1], (unsigned)nsub_max);
    uint2* in = st_in + (int64_t)blockIdx.x * nsub_max;
    uint2* out = st_out + (int64_t)blockIdx.x * nsub_max;
    unsigned* cnt = first + (int64_t)blockIdx.x * nsub_max;
    const int nluma = g.hs * g.hs;

    for (unsigned i = threadIdx.x; i < nsub; i += 256) in[i] = make_uint2(i * (unsigned)L, DIRTY);
    if (nsub <= 256) stage_window(s_win, words, 0, nwords);  // one window holds the image: staged once
    for (unsigned round = 0; round <= nsub; ++round) {       // nsub + 1 rounds: the hard limit
        for (unsigned i0 = 0; i0 < nsub; i0 += 256) {        // a window of 256 subsequences a trip
            const unsigned i = i0 + threadIdx.x;
            const uint2 v = i < nsub ? in[i] : make_uint2(0u, 0u);
            if (nsub > 256) {
                if (!__syncthreads_or((int)(v.y & DIRTY))) continue;          // (also ends the last trip's reads of the window)
                stage_window(s_win, words, i0 * WPS, nwords);
            }
            if (v.y & DIRTY) {
                dec_state s = unpack_state(v);
                null_sink sink;
                cnt[i] = decode_span(s_win, i0 * (unsigned)L, min((i + 1u) * (unsigned)L, nbits), s, s_tab, nluma, g.per_mcu, sink);
                out[i] = pack_state(s);
                in[i] = make_uint2(v.x, v.y & ~DIRTY);
            }
        }
        __syncthreads();
        int changed = 0;
        for (unsigned i = threadIdx.x; i < nsub; i += 256) {
            if (i == 0) continue;
            const uint2 o = out[i - 1], v = in[i];
            if (o.x != v.x || o.y != v.y) {
                in[i] = make_uint2(o.x, o.y | DIRTY);
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) break;
    }

    unsigned carry = 0;
    for (unsigned base = 0; base < nsub; base += 256) {
        const unsigned i = base + threadIdx.x;
        const unsigned v = i < nsub ? cnt[i] : 0u;
        unsigned total;
        const unsigned ex = block_scan(v, s_w, total);
        if (i < nsub) cnt[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0 && (int64_t)carry < g.nblk) atomicOr(status + blockIdx.x, -1);      // the data ended before the last block
}

// ------------------------------------------------------------------------------------------------ 3. emit
// One thread a subsequence of the batch; a workgroup takes 256 consecutive subsequences of one image (one window): blockIdx.x =
// image * nchunk + chunk, nchunk = ceil(nsub_max / 256).
__global__ __launch_bounds__(256) void emit_kernel(const unsigned char* __restrict__ clean, int64_t clean_stride,
                                                   const unsigned* __restrict__ meta, const unsigned char* __restrict__ huff,
                                                   const uint2* __restrict__ st_in, const unsigned* __restrict__ first,
                                                   short* __restrict__ coef_y, short* __restrict__ coef_c, int* __restrict__ dcd,
                                                   int* __restrict__ status, int nsub_max, int nchunk, scan_geom g) {
    __shared__ huff_dec s_tab[6];
    __shared__ unsigned s_win[WIN_LDS];
    const int64_t b = blockIdx.x / nchunk;
    const unsigned i0 = (unsigned)(blockIdx.x - b * nchunk) * 256u, i = i0 + threadIdx.x;
    const unsigned nbits = meta[2 * b], nsub = min(meta[2 * b + 1], (unsigned)nsub_max);
    if (i0 >= nsub) return;                                  // (the whole workgroup)
    build_tables(s_tab, huff, g.C);
    stage_window(s_win, reinterpret_cast<const unsigned*>(clean + b * clean_stride), i0 * WPS, (unsigned)(clean_stride / 4));
    if (i >= nsub) return;
    const int64_t gi = b * nsub_max + i;
    dec_state s = unpack_state(st_in[gi]);
    emit_sink sink{g, coef_y + b * g.bhn * g.bwn * 64, coef_c + b * 2 * g.nmcu * 64, dcd + b * g.nblk, status + b, (int64_t)first[gi]};
    sink.set_block();
    decode_span(s_win, i0 * (unsigned)L, min((i + 1u) * (unsigned)L, nbits), s, s_tab, g.hs * g.hs, g.per_mcu, sink);
}

// ------------------------------------------------------------------------------------------------ 4. DC
// One workgroup an image (blockIdx.x) and component (blockIdx.y): the running sum of the component's differences in scan order,
// dummies included, stored to coefficient 0 of the blocks that exist; a DC outside +-2047 flags the image.
__global__ __launch_bounds__(256) void dc_kernel(const int* __restrict__ dcd, short* __restrict__ coef_y, short* __restrict__ coef_c,
                                                 int* __restrict__ status, scan_geom g) {
    __shared__ unsigned s_w[4];
    const int64_t b = blockIdx.x;
    const int comp = blockIdx.y, nluma = g.hs * g.hs;
    const int64_t n = comp == 0 ? g.nmcu * nluma : g.nmcu;
    const int* d = dcd + b * g.nblk;
    unsigned carry = 0;
    bool bad = false;
    for (int64_t base = 0; base < n; base += 256) {
        const int64_t e = base + threadIdx.x;
        const bool live = e < n;
        const int64_t mcu = comp == 0 ? e / nluma : e;
        const int slot = comp == 0 ? (int)(e - mcu * nluma) : nluma + comp - 1;
        const unsigned v = live ? (unsigned)d[mcu * g.per_mcu + slot] : 0u;
        unsigned total;
        const int dc = (int)(carry + block_scan(v, s_w, total) + v);
        carry += total;
        if (!live) continue;
        bad = bad || dc < -2047 || dc > 2047;
        if (comp == 0) {
            const int my = (int)(mcu / g.mw), mx = (int)(mcu - (int64_t)my * g.mw);
            int by, bx;
            if (luma_source(g, my, mx, slot, by, bx)) coef_y[((b * g.bhn + by) * g.bwn + bx) * 64] = (short)dc;
        } else {
            coef_c[((b * 2 + comp - 1) * g.nmcu + mcu) * 64] = (short)dc;
        }
    }
    if (bad) atomicOr(status + b, -1);
}

// ------------------------------------------------------------------------------------------------ 5. pixels
// One plane's 8x8 block from its quantised coefficients (src: the block, looked at only where have) and its table tq, both at index
// 8 u + v: v = this lane's row r of samples 0..255.  Steps 7 of the file channel; lanes and LDS tile as block_roundtrip's second half.
// One workgroup barrier: every wave of the workgroup calls this the same number of times.
__device__ __forceinline__ void block_inverse(const short* __restrict__ src, bool have, const unsigned short* __restrict__ tq, int* iv, int r,
                                              int (&v)[8]) {
    int a[8], g[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] = have ? __mul24((int)src[u * 8 + r], (int)tq[u * 8 + r]) : 0;
    idct_pass<true>(a, g);
#pragma unroll
    for (int i = 0; i < 8; ++i) iv[i * 8 + r] = g[i];
    __syncthreads();
    const int4 v0 = reinterpret_cast<const int4*>(iv + r * 8)[0], v1 = reinterpret_cast<const int4*>(iv + r * 8)[1];
    a[0] = v0.x; a[1] = v0.y; a[2] = v0.z; a[3] = v0.w; a[4] = v1.x; a[5] = v1.y; a[6] = v1.z; a[7] = v1.w;
    idct_pass<false>(a, g);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = clamp_u8(g[j] + 128);
}

// 4:2:0, launch one: the decoded Cb and Cr at half resolution as bytes, half: uint8 [B][2][ch][cw].  qt: uint16 [B][3][64].
__global__ __launch_bounds__(256) void decode_chroma420_kernel(unsigned char* __restrict__ half, const short* __restrict__ coef_c,
                                                               const unsigned short* __restrict__ qt, int H, int W, int64_t ntiles) {
    __shared__ __attribute__((aligned(16))) int s_tile[4][8 * TILE_LD];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, blk = lane & 7, r = lane >> 3;
    int* iv = &s_tile[wave][blk * TILE_LD];
    const int ch = (H + 1) >> 1, cw = (W + 1) >> 1;
    const int cbwn = (cw + 7) >> 3, cbhn = (ch + 7) >> 3, txn = (cbwn + 7) >> 3;
    for (int64_t t0 = tile_first(); t0 < ntiles; t0 += tile_step()) {
        const jpeg_tile t(t0, wave, lane, ntiles, txn, cbhn, cbwn);          // the walk over CHROMA blocks
        const int64_t b = t.b;
        const bool have = t.bx < cbwn;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            int v[8];
            block_inverse(coef_c + (((b * 2 + p) * cbhn + t.by) * cbwn + t.bx) * 64, have, qt + (b * 3 + 1 + p) * 64, iv, r, v);
            if (t.live && t.yy < ch) {
                unsigned char* dst = half + ((b * 2 + p) * ch + t.yy) * cw + t.x0;
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (t.x0 + k < cw) dst[k] = (unsigned char)v[k];
            }
        }
    }
}

// The luma (C = 1: the only plane), with SUB == 0 and C == 3 the full-resolution chroma, with SUB == 2 the chroma from `half` through
// the upsampler; colour out and the store.  VEC: W % 8 == 0, out 8-byte and y 16-byte aligned.  qt: uint16 [B][C][64].
template <int C, int SUB, bool VEC>
__global__ __launch_bounds__(256) void decode_pixels_kernel(unsigned char* __restrict__ out, float* __restrict__ y,
                                                            const short* __restrict__ coef_y, const short* __restrict__ coef_c,
                                                            const unsigned char* __restrict__ half, const unsigned short* __restrict__ qt,
                                                            int H, int W, int64_t ntiles) {
    __shared__ __attribute__((aligned(16))) int s_tile[4][8 * TILE_LD];
    __shared__ float s_unit[256];                            // byte -> received f32
    fill_unit(s_unit);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, blk = lane & 7, r = lane >> 3;
    int* iv = &s_tile[wave][blk * TILE_LD];
    const int bwn = (W + 7) >> 3, bhn = (H + 7) >> 3, txn = (bwn + 7) >> 3;
    for (int64_t t0 = tile_first(); t0 < ntiles; t0 += tile_step()) {
        const jpeg_tile t(t0, wave, lane, ntiles, txn, bhn, bwn);
        const int64_t b = t.b;
        const bool have = t.bx < bwn;
        int pl[3][8];                                        // Y (Cb Cr), 0..255
        block_inverse(coef_y + ((b * bhn + t.by) * bwn + t.bx) * 64, have, qt + b * C * 64, iv, r, pl[0]);
        if constexpr (C == 3 && SUB == 0) {
#pragma unroll
            for (int p = 0; p < 2; ++p)
                block_inverse(coef_c + (((b * 2 + p) * bhn + t.by) * bwn + t.bx) * 64, have, qt + (b * 3 + 1 + p) * 64, iv, r, pl[1 + p]);
        }
        if constexpr (C == 3 && SUB == 2) IDEAS_UPSAMPLE420_ROW(half, b, H, W, t.yy, t.bx, pl)
        unsigned ob[8 * C];                                  // the bytes of this lane's row, pixel-major
        ycc_to_rgb<C>(pl, ob);
        if (t.live && t.yy < H) store8<C, VEC>(out, y, ((b * H + t.yy) * W + t.x0) * C, ob, t.x0, W, s_unit);
    }
}

// ------------------------------------------------------------------------------------------------ host side
// What a call needs, from its arguments; ok = false for arguments the decoder refuses.  B <= 0 plans one image.
struct dec_plan {
    bool ok = false;
    scan_geom g;
    int cap;                       // clean bytes kept of an image: what its blocks can need (208 each) or what a row holds
    int nsub_max;                  // subsequences of cap bytes
    int64_t clean_stride;          // cap + the 16 bytes of FF, a multiple of 16
    int64_t ntiles, ctiles;        // tiles of 8 blocks of the pixel launches (luma grid; chroma grid at 4:2:0, else 0)
    // the workspace behind its 16-byte alignment
    size_t clean_at, meta_at, in_at, out_at, first_at, dcd_at, coefy_at, coefc_at, half_at, bytes;
    size_t coefy_bytes, coefc_bytes;
};

size_t up16(size_t v) { return (v + 15) / 16 * 16; }

dec_plan plan_for(int B, int C, int H, int W, int sub, long long row_stride) {
    dec_plan p;
    if ((C != 1 && C != 3) || H <= 0 || W <= 0 || H > 65535 || W > 65535 || (sub != 0 && sub != 2) || row_stride < 1) return p;
    p.g = make_scan_geom(C, H, W, sub);
    const scan_geom& g = p.g;
    const int64_t nb = B > 0 ? B : 1;
    const int64_t cap = std::min<int64_t>(row_stride, 208 * g.nblk + 8);
    if (cap > (INT32_MAX >> 3) - 2 * L || nb * g.nblk > INT32_MAX) return p;          // bit positions and block indices are 32-bit
    p.cap = (int)cap;
    p.nsub_max = (int)ideas_cdiv(cap * 8, L);
    if (nb * (ideas_cdiv(p.nsub_max, 256) * 256) > INT32_MAX) return p;
    p.clean_stride = (int64_t)up16((size_t)cap + 16);
    p.ntiles = nb * g.bhn * ideas_cdiv(g.bwn, 8);
    const int64_t ch = (H + 1) / 2, cw = (W + 1) / 2;
    p.ctiles = g.hs == 2 ? nb * ideas_cdiv(ch, 8) * ideas_cdiv(ideas_cdiv(cw, 8), 8) : 0;
    if (ideas_cdiv(p.ntiles, 4) > INT32_MAX) return p;
    const size_t n = (size_t)nb, ns = n * (size_t)p.nsub_max;
    p.coefy_bytes = n * (size_t)g.bhn * (size_t)g.bwn * 128;
    p.coefc_bytes = C == 3 ? n * 2 * (size_t)g.nmcu * 128 : 0;
    p.clean_at = 0;
    p.meta_at = p.clean_at + n * (size_t)p.clean_stride;
    p.in_at = up16(p.meta_at + n * 8);
    p.out_at = up16(p.in_at + ns * 8);
    p.first_at = up16(p.out_at + ns * 8);
    p.dcd_at = up16(p.first_at + ns * 4);
    p.coefy_at = up16(p.dcd_at + n * (size_t)g.nblk * 4);
    p.coefc_at = up16(p.coefy_at + p.coefy_bytes);
    p.half_at = up16(p.coefc_at + p.coefc_bytes);
    p.bytes = up16(p.half_at + (g.hs == 2 ? n * 2 * (size_t)ch * (size_t)cw : 0)) + 16;     // 16: a workspace that arrives unaligned
    p.ok = true;
    return p;
}

template <int C, int SUB>
void launch_pixels(void* out, float* y, const short* coef_y, const short* coef_c, unsigned char* half, const unsigned short* qt,
                   const dec_plan& p, int H, int W, hipStream_t stream) {
    if constexpr (C == 3 && SUB == 2)
        hipLaunchKernelGGL(decode_chroma420_kernel, dim3((unsigned)ideas_cdiv(p.ctiles, 4)), dim3(256), 0, stream, half, coef_c, qt, H, W,
                           p.ctiles);
    const dim3 grid((unsigned)ideas_cdiv(p.ntiles, 4));
    if (W % 8 == 0 && ideas_aligned<8>(out) && ideas_aligned16(y))
        hipLaunchKernelGGL((decode_pixels_kernel<C, SUB, true>), grid, dim3(256), 0, stream, (unsigned char*)out, y, coef_y, coef_c,
                           (const unsigned char*)half, qt, H, W, p.ntiles);
    else
        hipLaunchKernelGGL((decode_pixels_kernel<C, SUB, false>), grid, dim3(256), 0, stream, (unsigned char*)out, y, coef_y, coef_c,
                           (const unsigned char*)half, qt, H, W, p.ntiles);
}

}  // namespace

extern "C" size_t ideas_jpeg_file_decode_workspace_bytes(int B, int C, int H, int W, int subsampling, long long row_stride) {
    if (B <= 0) return 0;
    const dec_plan p = plan_for(B, C, H, W, subsampling, row_stride);
    return p.ok ? p.bytes : 0;
}

extern "C" int ideas_jpeg_file_decode(void* out_u8, float* y, short* coef_y, short* coef_c, int* status, const void* scans,
                                      const int* nbytes, long long row_stride, const unsigned short* qt, const unsigned char* huff,
                                      void* workspace, int B, int C, int H, int W, int subsampling, void* stream_) {
    if (!out_u8 || !status || !scans || !nbytes || !qt || !huff || !workspace) return IDEAS_E_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || H > 65535 || W > 65535 || (C != 1 && C != 3) || row_stride < 1) return IDEAS_E_SHAPE;
    if (subsampling != 0 && subsampling != 2) return IDEAS_E_UNSUPPORTED;
    const dec_plan p = plan_for(B, C, H, W, subsampling, row_stride);
    if (!p.ok) return IDEAS_E_SHAPE;
    hipStream_t stream = (hipStream_t)stream_;
    const scan_geom& g = p.g;

    unsigned char* base = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(workspace) + 15) & ~(uintptr_t)15);
    unsigned char* clean = base + p.clean_at;
    unsigned* meta = reinterpret_cast<unsigned*>(base + p.meta_at);
    uint2* st_in = reinterpret_cast<uint2*>(base + p.in_at);
    uint2* st_out = reinterpret_cast<uint2*>(base + p.out_at);
    unsigned* first = reinterpret_cast<unsigned*>(base + p.first_at);
    int* dcd = reinterpret_cast<int*>(base + p.dcd_at);
    unsigned char* half = base + p.half_at;
    // the zeros of the coefficient arrays (the caller's, or the workspace's copies in one stretch) and of the flags
    hipError_t e = hipMemsetAsync(status, 0, (size_t)B * 4, stream);
    if (e == hipSuccess && !coef_y && !(C == 3 && coef_c)) {
        e = hipMemsetAsync(base + p.coefy_at, 0, p.coefc_at + p.coefc_bytes - p.coefy_at, stream);
        coef_y = reinterpret_cast<short*>(base + p.coefy_at);
        coef_c = reinterpret_cast<short*>(base + p.coefc_at);
    } else {
        if (!coef_y) coef_y = reinterpret_cast<short*>(base + p.coefy_at);
        if (C == 3 && !coef_c) coef_c = reinterpret_cast<short*>(base + p.coefc_at);
        if (e == hipSuccess) e = hipMemsetAsync(coef_y, 0, p.coefy_bytes, stream);
        if (e == hipSuccess && C == 3) e = hipMemsetAsync(coef_c, 0, p.coefc_bytes, stream);
    }
    if (e != hipSuccess) return (int)e;
    if (C == 1) coef_c = reinterpret_cast<short*>(base + p.coefc_at);          // never dereferenced

    hipLaunchKernelGGL(unstuff_kernel, dim3(B), dim3(256), 0, stream, (const unsigned char*)scans, nbytes, (int64_t)row_stride, clean,
                       p.clean_stride, p.cap, meta, status);
    hipLaunchKernelGGL(sync_kernel, dim3(B), dim3(256), 0, stream, (const unsigned char*)clean, p.clean_stride, (const unsigned*)meta,
                       huff, st_in, st_out, first, status, p.nsub_max, g);
    const int nchunk = (int)ideas_cdiv(p.nsub_max, 256);
    hipLaunchKernelGGL(emit_kernel, dim3((unsigned)((int64_t)B * nchunk)), dim3(256), 0, stream, (const unsigned char*)clean,
                       p.clean_stride, (const unsigned*)meta, huff, (const uint2*)st_in, (const unsigned*)first, coef_y, coef_c, dcd,
                       status, p.nsub_max, nchunk, g);
    hipLaunchKernelGGL(dc_kernel, dim3(B, C), dim3(256), 0, stream, (const int*)dcd, coef_y, coef_c, status, g);
    int rc = ideas_launch_status();
    if (rc != IDEAS_OK) return rc;
    if (C == 1)
        launch_pixels<1, 0>(out_u8, y, coef_y, coef_c, half, qt, p, H, W, stream);
    else if (subsampling == 2)
        launch_pixels<3, 2>(out_u8, y, coef_y, coef_c, half, qt, p, H, W, stream);
    else
        launch_pixels<3, 0>(out_u8, y, coef_y, coef_c, half, qt, p, H, W, stream);
    return ideas_launch_status();
}
