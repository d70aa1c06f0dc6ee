// The PNG FILE, written on the device: from the uint8 container [B, H, W, C] of ideas_image_f32_to_u8 to a file any PNG reader opens --
// row filters, a deflate stream of Huffman-coded literals (no matches), Adler-32 and the chunk CRCs.  The file is stated in
// include/ideas_hip.h ("The PNG file, written") and restated in numpy by tests/png_ref.py, which tests/test_png_file.py holds to zlib's
// inflate and to Pillow's reader.
//
// A code has a variable length and every stripe of IDEAS_PNG_STRIPE_ROWS rows its own code, so the file is made in four launches behind
// one memset:
//   filter_kernel   one workgroup a row: the five residual rows' costs, the choice, the filtered row, and the row's histogram added to
//                   its stripe's (LDS atomics, then one global add a bin in use).
//   tables_kernel   one wave a stripe: the length-limited code of the stripe's histogram (build_code: rank the leaves, one lane merges
//                   them, every lane walks its leaves up to the root, the counts per length are repaired and handed out), the code of
//                   those lengths, the bits of the block header and the stripe's bit count.
//   pack_kernel     one workgroup a stripe: its bit offset (the sum of the counts of the stripes before it), the header, then 4096
//                   bytes a trip, 16 a thread: a workgroup prefix sum of the code lengths places every thread's run, which is written
//                   into a cleared buffer of 32-bit words (a run's first and last word, shared with its neighbours, by atomicOr).
//                   Counting and writing are ONE function (emit_run) over two sinks.
//   finish_kernel   one workgroup an image: Adler-32 of the filtered bytes and CRC-32 of IDAT from per-thread slices, the chunk
//                   framing, the copy of the stream into the file, and the length.
// No store is addressed by data: every index is derived from the shape.  DESIGN.md 3.15.1b.
#include "u8.hpp"
#include "jpeg_scan.hpp"

namespace {

constexpr int STRIPE = IDEAS_PNG_STRIPE_ROWS;
constexpr int NLIT = 257;          // literals 0..255 and the end-of-block symbol
constexpr int CODE_LD = 260;       // words from one stripe's code table (symbol -> reversed code | length << 16) to the next
constexpr int HDR_BITS = 17 + 19 * 3 + 258 * 7;       // the longest block header: 7 bits a code length
constexpr int HDR_WORDS = 64;      // words from one stripe's header bits to the next (HDR_BITS = 1880: 59 words)
constexpr int PACK_RUN = 16, PACK_TILE = 256 * PACK_RUN;
constexpr int FILE_HEAD = 8 + 25 + 8 + 2;             // signature, IHDR, IDAT's length and type, 78 01
constexpr int FILE_REST = 4 + 4 + 12;                 // Adler-32, IDAT's CRC, IEND
static_assert(HDR_BITS <= HDR_WORDS * 32, "a block header fits its slot");

// ------------------------------------------------------------------------------------------------ checksums
// CRC-32 (reflected, polynomial EDB88320) on the register BEFORE the final inversion: a byte, a product modulo the polynomial
// (bit 31 is x^0), and x^(8 n).  A slice's register started from 0 is linear in the bytes, so the register of a whole message is
// the XOR of its slices' registers, each multiplied by x^(8 * bytes behind the slice).
constexpr unsigned CRC_POLY = 0xedb88320u;
__host__ __device__ constexpr unsigned crc_byte(unsigned s, unsigned byte) {
    s ^= byte;
    for (int k = 0; k < 8; ++k) s = (s >> 1) ^ (CRC_POLY & (0u - (s & 1u)));
    return s;
}
__host__ __device__ constexpr unsigned crc_mul(unsigned a, unsigned b) {
    unsigned p = 0;
    for (int k = 0; k < 32; ++k) {
        p ^= b & (0u - ((a >> (31 - k)) & 1u));
        b = (b >> 1) ^ (CRC_POLY & (0u - (b & 1u)));
    }
    return p;
}
struct crc_powers {
    unsigned v[32];                // x^(2^k)
};
constexpr crc_powers make_crc_powers() {
    crc_powers t = {};
    t.v[0] = 1u << 30;
    for (int k = 1; k < 32; ++k) t.v[k] = crc_mul(t.v[k - 1], t.v[k - 1]);
    return t;
}
constexpr crc_powers K_CRC_POWERS = make_crc_powers();
__device__ const crc_powers k_crc_powers = K_CRC_POWERS;
// x^(8 n), n < 2^61
template <class Table> __host__ __device__ constexpr unsigned crc_xpow8(uint64_t n, const Table& t) {
    unsigned p = 1u << 31;
    for (int k = 3; n; n >>= 1, ++k)
        if (n & 1u) p = crc_mul(t.v[k & 31], p);
    return p;
}
constexpr unsigned crc_of(const char* s, int n, unsigned state) {
    for (int i = 0; i < n; ++i) state = crc_byte(state, (unsigned char)s[i]);
    return state;
}
constexpr unsigned K_IEND_CRC = ~crc_of("IEND", 4, 0xffffffffu);
constexpr unsigned K_IDAT_STATE = crc_of("IDAT\x78\x01", 6, 0xffffffffu);      // the register in front of the deflate stream
static_assert(K_IEND_CRC == 0xae426082u, "CRC-32 of IEND");
static_assert((crc_mul(crc_xpow8(2, K_CRC_POWERS), crc_of("IE", 2, 0xffffffffu)) ^ crc_of("ND", 2, 0u)) == crc_of("IEND", 4, 0xffffffffu),
              "two slices combine to the whole");
static_assert(crc_xpow8(4, K_CRC_POWERS) == K_CRC_POWERS.v[5], "x^32");

constexpr unsigned ADLER_MOD = 65521u;

// ------------------------------------------------------------------------------------------------ filters
__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// the residuals of byte i of a row under the five filters; up: the raw row above or null; bpp = C
__device__ __forceinline__ void residuals(const unsigned char* __restrict__ row, const unsigned char* __restrict__ up, int64_t i, int C,
                                          unsigned (&r)[5]) {
    const int x = row[i];
    const int a = i >= C ? row[i - C] : 0;
    const int b = up ? up[i] : 0;
    const int c = (up && i >= C) ? up[i - C] : 0;
    r[0] = (unsigned)x;
    r[1] = (unsigned)(x - a) & 255u;
    r[2] = (unsigned)(x - b) & 255u;
    r[3] = (unsigned)(x - ((a + b) >> 1)) & 255u;
    r[4] = (unsigned)(x - paeth(a, b, c)) & 255u;
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
    return v;
}

// One workgroup a row (blockIdx.x = b * H + y).  filt: [B][H][n + 1], the type byte in front of the n = W * C residuals; hist:
// [B][ns][256], cleared.
__global__ __launch_bounds__(256) void filter_kernel(unsigned char* __restrict__ filt, unsigned* __restrict__ hist,
                                                     const unsigned char* __restrict__ u8, int H, int64_t n, int C, int ns) {
    __shared__ unsigned s_hist[256];
    __shared__ uint64_t s_cost[4][5];
    const int64_t row = blockIdx.x;
    const int64_t b = row / H;
    const int y = (int)(row - b * H);
    const unsigned char* src = u8 + row * n;
    const unsigned char* up = y > 0 ? src - n : nullptr;
    s_hist[threadIdx.x] = 0;

    unsigned cost[5] = {0, 0, 0, 0, 0};                       // at most 128 a byte, n / 256 + 1 bytes: 32 bits hold it
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        unsigned r[5];
        residuals(src, up, i, C, r);
#pragma unroll
        for (int k = 0; k < 5; ++k) cost[k] += r[k] < 128u ? r[k] : 256u - r[k];
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const uint64_t w = wave_sum_u64(cost[k]);
        if ((threadIdx.x & 63) == 0) s_cost[threadIdx.x >> 6][k] = w;
    }
    __syncthreads();
    int type = 0;
    uint64_t best = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const uint64_t t = s_cost[0][k] + s_cost[1][k] + s_cost[2][k] + s_cost[3][k];
        if (k == 0 || t < best) {                             // a tie goes to the lowest type
            best = t;
            type = k;
        }
    }

    unsigned char* dst = filt + row * (n + 1);
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        unsigned r[5];
        residuals(src, up, i, C, r);
        const unsigned v = type == 0 ? r[0] : type == 1 ? r[1] : type == 2 ? r[2] : type == 3 ? r[3] : r[4];
        dst[1 + i] = (unsigned char)v;
        atomicAdd(&s_hist[v], 1u);
    }
    if (threadIdx.x == 0) {
        dst[0] = (unsigned char)type;
        atomicAdd(&s_hist[type], 1u);
    }
    __syncthreads();
    const unsigned v = s_hist[threadIdx.x];
    if (v) atomicAdd(hist + ((b * ns + y / STRIPE) * 256 + threadIdx.x), v);
}

// ------------------------------------------------------------------------------------------------ codes
__device__ const unsigned char k_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// build_code's working arrays, for up to NLIT symbols
struct code_lds {
    unsigned w[2 * NLIT];          // node weights: the leaves in ascending (frequency, symbol), then the internal nodes as made
    unsigned short parent[2 * NLIT];
    unsigned short order[NLIT + 1];                           // leaf -> symbol
    unsigned char len[NLIT + 3];   // symbol -> length
    unsigned count[16];            // codes of each length
};

// One wave (the whole workgroup: the barriers are the workgroup's): the length-limited canonical code of freq[0 .. nsym) as stated in
// include/ideas_hip.h -> code[sym] = reversed code | length << 16, 0 for an unused symbol; t.len and t.count are left for the caller.
template <int MAXBITS> __device__ void build_code(const unsigned* freq, int nsym, unsigned* code, code_lds& t) {
    const int lane = threadIdx.x;
    // the leaves in order: a used symbol's rank is the number of used symbols in front of it
    int n = 0;
    for (int base = 0; base < nsym; base += 64) {
        const int i = base + lane;
        const unsigned f = i < nsym ? freq[i] : 0u;
        n += __popcll(__ballot(f != 0u));
        if (i < nsym) t.len[i] = 0;
        if (f != 0u) {
            int r = 0;
            for (int j = 0; j < nsym; ++j) {
                const unsigned g = freq[j];
                r += (g != 0u && (g < f || (g == f && j < i))) ? 1 : 0;
            }
            t.order[r] = (unsigned short)i;
            t.w[r] = f;
        }
    }
    if (lane < 16) t.count[lane] = 0;
    __syncthreads();
    // the two lightest nodes are merged; a leaf goes before an internal node of the same weight
    if (lane == 0) {
        int li = 0, ii = n, next = n;
        for (int k = 0; k + 1 < n; ++k) {
            int pick[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const bool leaf = li < n && (ii >= next || t.w[li] <= t.w[ii]);
                pick[e] = leaf ? li : ii;
                li += leaf ? 1 : 0;
                ii += leaf ? 0 : 1;
            }
            t.w[next] = t.w[pick[0]] + t.w[pick[1]];
            t.parent[pick[0]] = (unsigned short)next;
            t.parent[pick[1]] = (unsigned short)next;
            ++next;
        }
    }
    __syncthreads();
    // a leaf's depth, counted at the limit where it is deeper
    const int root = 2 * n - 2;
    for (int r = lane; r < n; r += 64) {
        int d = 0;
        for (int k = r; k != root && d < 2 * NLIT; ++d) k = t.parent[k];
        atomicAdd(&t.count[min(max(d, 1), MAXBITS)], 1u);
    }
    __syncthreads();
    // while the Kraft sum is over 1: one unit of 2^-MAXBITS less a step
    if (lane == 0) {
        int over = -(1 << MAXBITS);
        for (int l = 1; l <= MAXBITS; ++l) over += (int)(t.count[l] << (MAXBITS - l));
        for (; over > 0; --over) {
            int bits = MAXBITS - 1;
            while (bits > 0 && t.count[bits] == 0) --bits;
            if (bits == 0 || t.count[MAXBITS] == 0) break;    // (cannot happen: the counts came from a tree)
            t.count[bits] -= 1;
            t.count[bits + 1] += 2;
            t.count[MAXBITS] -= 1;
        }
    }
    __syncthreads();
    // the counts handed out in leaf order, the longest lengths to the lightest leaves
    for (int r = lane; r < n; r += 64) {
        int l = 0, cum = 0;
#pragma unroll
        for (int k = MAXBITS; k >= 1; --k) {
            cum += (int)t.count[k];
            if (l == 0 && r < cum) l = k;
        }
        t.len[t.order[r]] = (unsigned char)l;
    }
    __syncthreads();
    // canonical codes (RFC 1951 3.2.2), bit-reversed: every lane keeps the next code of each length
    unsigned next[MAXBITS + 1];
    next[0] = 0;
    {
        unsigned c = 0;
#pragma unroll
        for (int l = 1; l <= MAXBITS; ++l) {
            c = (c + (l > 1 ? t.count[l - 1] : 0u)) << 1;
            next[l] = c;
        }
    }
    for (int base = 0; base < nsym; base += 64) {
        const int i = base + lane;
        const int l = i < nsym ? (int)t.len[i] : 0;
        unsigned c = 0;
#pragma unroll
        for (int k = 1; k <= MAXBITS; ++k) {
            const uint64_t mask = __ballot(l == k);
            if (l == k) c = next[k] + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
            next[k] += (unsigned)__popcll(mask);
        }
        if (i < nsym) code[i] = l ? ((__brev(c) >> (32 - l)) | ((unsigned)l << 16)) : 0u;
    }
    __syncthreads();
}

// Bits from bit offset `off` of a cleared buffer of little-endian words, least significant bit first (RFC 1951 3.1.1).  acc holds
// `fill` < 32 pending bits above the zeros that stand for the bits in front of `off` in the first word; that word and the last one are
// shared with other writers and go out by atomicOr.
struct bit_writer {
    unsigned* w;
    uint64_t acc = 0;
    int fill;
    bool shared;
    __device__ __forceinline__ bit_writer(unsigned* words, uint64_t off) : w(words + (off >> 5)), fill((int)(off & 31u)), shared(fill != 0) {}
    __device__ __forceinline__ void put(unsigned v, int nbits) {                   // nbits <= 32, v < 2^nbits
        acc |= (uint64_t)v << fill;
        fill += nbits;
        if (fill >= 32) {
            if (shared) atomicOr(w, (unsigned)acc); else *w = (unsigned)acc;
            shared = false;
            acc >>= 32;
            fill -= 32;
            ++w;
        }
    }
    __device__ __forceinline__ void finish() {
        if (fill > 0) atomicOr(w, (unsigned)acc);
    }
};
struct bit_counter {
    unsigned n = 0;
    __device__ __forceinline__ void put(unsigned, int nbits) { n += (unsigned)nbits; }
};

// One wave a stripe (blockIdx.x = b * ns + s): codes[stripe][sym], the header's bits in hdr[stripe][...] with hbits[stripe] their
// number, and sbits[stripe] = the bits of the whole block.
__global__ __launch_bounds__(64) void tables_kernel(unsigned* __restrict__ codes, unsigned* __restrict__ hdr, unsigned* __restrict__ hbits,
                                                    uint64_t* __restrict__ sbits, const unsigned* __restrict__ hist, int ns) {
    __shared__ unsigned s_freq[NLIT + 3], s_code[NLIT + 3], s_clfreq[20], s_clcode[20];
    __shared__ code_lds t;
    const int lane = threadIdx.x;
    const int64_t gi = blockIdx.x;
    for (int i = lane; i < 256; i += 64) s_freq[i] = hist[gi * 256 + i];
    if (lane == 0) s_freq[256] = 1;                           // the end of the block, once
    if (lane < 20) s_clfreq[lane] = 0;
    __syncthreads();
    build_code<15>(s_freq, NLIT, s_code, t);

    uint64_t bits = 0;
    for (int i = lane; i < NLIT; i += 64) {
        const unsigned e = s_code[i];
        codes[gi * CODE_LD + i] = e;
        bits += (uint64_t)s_freq[i] * (e >> 16);
        atomicAdd(&s_clfreq[e >> 16], 1u);                    // no run-length symbols: every length is sent as itself
    }
    bits = wave_sum_u64(bits);
    if (lane == 0) atomicAdd(&s_clfreq[1], 1u);               // the one distance code, of length 1
    __syncthreads();
    build_code<7>(s_clfreq, 19, s_clcode, t);

    if (lane == 0) {
        int ncl = 4;
        for (int k = 4; k < 19; ++k)
            if (t.len[k_cl_order[k]]) ncl = k + 1;
        bit_writer out(hdr + gi * HDR_WORDS, 0);              // this stripe's own words, from bit 0: plain stores only
        bit_counter cnt;
        const unsigned final = (int)(gi % ns) == ns - 1 ? 1u : 0u;
        auto both = [&](unsigned v, int nb) {
            out.put(v, nb);
            cnt.put(v, nb);
        };
        both(final | (2u << 1), 3);                           // BFINAL, BTYPE = 2
        both(0u, 5);                                          // HLIT: 257 codes
        both(0u, 5);                                          // HDIST: 1 code
        both((unsigned)(ncl - 4), 4);
        for (int k = 0; k < ncl; ++k) both(t.len[k_cl_order[k]], 3);
        for (int i = 0; i < NLIT; ++i) {
            const unsigned e = s_clcode[s_code[i] >> 16];
            both(e & 0xffffu, (int)(e >> 16));
        }
        both(s_clcode[1] & 0xffffu, (int)(s_clcode[1] >> 16));
        if (out.fill > 0) *out.w = (unsigned)out.acc;         // the last word, plainly: nobody shares it
        hbits[gi] = cnt.n;
        sbits[gi] = bits + cnt.n;
    }
}

// A thread's run: cnt entries e[j] = reversed code | length << 16, then the end-of-block code where the run ends the stripe.
template <class Sink> __device__ __forceinline__ void emit_run(Sink& sink, const unsigned (&e)[PACK_RUN], int cnt, bool last, unsigned eob) {
#pragma unroll
    for (int j = 0; j < PACK_RUN; ++j)
        if (j < cnt) sink.put(e[j] & 0xffffu, (int)(e[j] >> 16));
    if (last) sink.put(eob & 0xffffu, (int)(eob >> 16));
}

// One workgroup a stripe (blockIdx.x = b * ns + s): its block at its bit offset of stream + b * words.
__global__ __launch_bounds__(256) void pack_kernel(unsigned* __restrict__ stream, int64_t words, const unsigned char* __restrict__ filt,
                                                   const unsigned* __restrict__ codes, const unsigned* __restrict__ hdr,
                                                   const unsigned* __restrict__ hbits, const uint64_t* __restrict__ sbits, int H,
                                                   int64_t n1, int ns) {
    __shared__ unsigned s_code[NLIT + 3], s_w[4];
    __shared__ uint64_t s_sum[4];
    const int64_t gi = blockIdx.x;
    const int64_t b = gi / ns;
    const int s = (int)(gi - b * ns);
    for (int i = threadIdx.x; i < NLIT; i += 256) s_code[i] = codes[gi * CODE_LD + i];
    uint64_t part = 0;
    for (int j = threadIdx.x; j < s; j += 256) part += sbits[b * ns + j];
    part = wave_sum_u64(part);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = part;
    __syncthreads();
    const uint64_t base = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    unsigned* out = stream + b * words;

    const unsigned hb = hbits[gi];
    if (threadIdx.x == 0) {
        bit_writer w(out, base);
        const unsigned* h = hdr + gi * HDR_WORDS;
        for (unsigned k = 0; k < (hb >> 5); ++k) w.put(h[k], 32);
        if (hb & 31u) w.put(h[hb >> 5] & ((1u << (hb & 31u)) - 1u), (int)(hb & 31u));
        w.finish();
    }

    const int rows = min(STRIPE, H - s * STRIPE);
    const int64_t S = (int64_t)rows * n1;
    const unsigned char* src = filt + (b * H + (int64_t)s * STRIPE) * n1;
    const unsigned eob = s_code[256];
    uint64_t at = base + hb;
    for (int64_t t0 = 0; t0 < S; t0 += PACK_TILE) {
        const int64_t i0 = t0 + threadIdx.x * PACK_RUN;
        const int cnt = (int)max((int64_t)0, min((int64_t)PACK_RUN, S - i0));
        const bool last = cnt > 0 && i0 + cnt == S;
        unsigned e[PACK_RUN];
#pragma unroll
        for (int j = 0; j < PACK_RUN; ++j) e[j] = j < cnt ? s_code[src[i0 + j]] : 0u;
        bit_counter count;
        emit_run(count, e, cnt, last, eob);
        unsigned total;
        const unsigned off = block_scan(count.n, s_w, total);
        if (cnt > 0) {
            bit_writer w(out, at + off);
            emit_run(w, e, cnt, last, eob);
            w.finish();
        }
        at += total;
    }
}

// ------------------------------------------------------------------------------------------------ the file
__device__ __forceinline__ unsigned be_byte(unsigned v, int k) { return (v >> (24 - 8 * k)) & 255u; }       // byte k of v, big-endian

// One workgroup of FIN_THREADS an image: the file from the stream of pack_kernel and the filtered bytes.  Both checksums are serial in a
// thread's slice, so the workgroup is as large as it can be.
constexpr int FIN_THREADS = 1024, FIN_WAVES = FIN_THREADS / 64;
template <class T> __device__ __forceinline__ T fin_sum(const T (&v)[FIN_WAVES]) {
    T s = 0;
#pragma unroll
    for (int i = 0; i < FIN_WAVES; ++i) s += v[i];
    return s;
}
__global__ __launch_bounds__(FIN_THREADS) void finish_kernel(unsigned char* __restrict__ files, int* __restrict__ nbytes, int64_t row_stride,
                                                     const unsigned char* __restrict__ stream, int64_t stream_stride,
                                                     const unsigned char* __restrict__ filt, const uint64_t* __restrict__ sbits, int C,
                                                     int H, int W, int ns) {
    __shared__ uint64_t s_sum[FIN_WAVES];
    __shared__ unsigned s_a[FIN_WAVES], s_b[FIN_WAVES], s_x[FIN_WAVES];
    __shared__ unsigned s_head[FILE_HEAD];
    const int64_t b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned char* out = files + b * row_stride;
    const unsigned char* in = stream + b * stream_stride;

    uint64_t part = 0;
    for (int j = threadIdx.x; j < ns; j += FIN_THREADS) part += sbits[b * ns + j];
    part = wave_sum_u64(part);
    if (lane == 0) s_sum[wave] = part;

    // Adler-32 of the filtered bytes: a slice from (0, 0) gives (a, b); behind it `after` bytes add a * after to b
    const int64_t N = (int64_t)H * ((int64_t)W * C + 1);
    const unsigned char* fb = filt + b * N;
    {
        const int64_t L = (N + FIN_THREADS - 1) / FIN_THREADS, lo = min(N, threadIdx.x * L), hi = min(N, lo + L);
        uint64_t a = 0, bb = 0;
        for (int64_t i0 = lo; i0 < hi; i0 += 4096) {          // 4096 bytes keep both sums far inside 64 bits
            const int64_t i1 = min(hi, i0 + 4096);
            for (int64_t i = i0; i < i1; ++i) {
                a += fb[i];
                bb += a;
            }
            a %= ADLER_MOD;
            bb %= ADLER_MOD;
        }
        bb = (bb + a * (uint64_t)((N - hi) % ADLER_MOD)) % ADLER_MOD;
        unsigned ra = (unsigned)a, rb = (unsigned)bb;        // FIN_THREADS of them: 32 bits hold the sums
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            ra += __shfl_xor(ra, o, 64);
            rb += __shfl_xor(rb, o, 64);
        }
        if (lane == 0) {
            s_a[wave] = ra;
            s_b[wave] = rb;
        }
    }
    __syncthreads();
    const uint64_t nd = (fin_sum(s_sum) + 7) >> 3;          // bytes of the deflate stream
    const unsigned adler_a = (unsigned)((1u + (uint64_t)fin_sum(s_a)) % ADLER_MOD);
    const unsigned adler_b = (unsigned)(((uint64_t)(N % ADLER_MOD) + fin_sum(s_b)) % ADLER_MOD);
    const unsigned adler = (adler_b << 16) | adler_a;

    // the head: signature, IHDR with its CRC, IDAT's length and type, 78 01
    if (threadIdx.x == 0) {
        const unsigned char sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
        for (int i = 0; i < 8; ++i) s_head[i] = sig[i];
        const unsigned idat_len = (unsigned)(2 + nd + 4);
        for (int k = 0; k < 4; ++k) {
            s_head[8 + k] = be_byte(13u, k);
            s_head[12 + k] = (unsigned char)"IHDR"[k];
            s_head[16 + k] = be_byte((unsigned)W, k);
            s_head[20 + k] = be_byte((unsigned)H, k);
            s_head[33 + k] = be_byte(idat_len, k);
            s_head[37 + k] = (unsigned char)"IDAT"[k];
        }
        s_head[24] = 8;                                       // bit depth
        s_head[25] = C == 3 ? 2 : 0;                          // colour type
        s_head[26] = s_head[27] = s_head[28] = 0;             // compression, filter, interlace
        unsigned crc = 0xffffffffu;
        for (int i = 12; i < 29; ++i) crc = crc_byte(crc, s_head[i]);
        for (int k = 0; k < 4; ++k) s_head[29 + k] = be_byte(~crc, k);
        s_head[41] = 0x78;
        s_head[42] = 0x01;
    }

    // CRC-32 of IDAT: thread 0's slice starts from the register behind "IDAT" 78 01, the others from 0
    {
        const int64_t n = (int64_t)nd, L = (n + FIN_THREADS - 1) / FIN_THREADS, lo = min(n, threadIdx.x * L), hi = min(n, lo + L);
        unsigned state = threadIdx.x == 0 ? K_IDAT_STATE : 0u;
        for (int64_t i = lo; i < hi; ++i) state = crc_byte(state, in[i]);
        unsigned x = crc_mul(crc_xpow8((uint64_t)(n - hi), k_crc_powers), state);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x ^= __shfl_xor(x, o, 64);
        if (lane == 0) s_x[wave] = x;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < FILE_HEAD; i += FIN_THREADS) out[i] = (unsigned char)s_head[i];
    for (int64_t i = threadIdx.x; i < (int64_t)nd; i += FIN_THREADS) out[FILE_HEAD + i] = in[i];
    if (threadIdx.x == 0) {
        unsigned char* p = out + FILE_HEAD + nd;
        unsigned crc = 0;
        for (int i = 0; i < FIN_WAVES; ++i) crc ^= s_x[i];
        for (int k = 0; k < 4; ++k) {
            p[k] = (unsigned char)be_byte(adler, k);
            crc = crc_byte(crc, be_byte(adler, k));
        }
        for (int k = 0; k < 4; ++k) {
            p[4 + k] = (unsigned char)be_byte(~crc, k);
            p[8 + k] = 0;                                     // IEND: no data
            p[12 + k] = (unsigned char)"IEND"[k];
            p[16 + k] = (unsigned char)be_byte(K_IEND_CRC, k);
        }
        nbytes[b] = (int)(FILE_HEAD + nd + FILE_REST);
    }
}

// What a call needs, from its arguments; ok = false for arguments the writer refuses (shape, or a size beyond an int of bytes a file
// or of rows a launch).  B <= 0 plans one image.
struct png_plan {
    bool ok = false;
    int ns;                        // stripes an image
    int64_t n1;                    // filtered bytes a row
    int64_t max_bytes;             // every symbol at most 15 bits, every header at most HDR_BITS
    int64_t stream_stride;         // bytes of one image's deflate stream and a word to spare, a multiple of 16
    size_t codes_at, hdr_at, hbits_at, sbits_at, cleared_at, stream_at, bytes;      // the workspace behind its alignment: filt first
};

size_t up16(size_t v) { return (v + 15) / 16 * 16; }

png_plan plan_for(int B, int C, int H, int W) {
    png_plan p;
    if ((C != 1 && C != 3) || H <= 0 || W <= 0) return p;
    p.ns = (int)ideas_cdiv(H, STRIPE);
    p.n1 = (int64_t)W * C + 1;
    const int64_t nb = B > 0 ? B : 1;
    if (p.n1 > INT32_MAX || (int64_t)H * p.n1 > INT32_MAX) return p;              // (keeps the products below inside 64 bits)
    const int64_t bits = (int64_t)p.ns * (HDR_BITS + 15) + 15 * (int64_t)H * p.n1;
    const int64_t nd = (bits + 7) / 8;
    p.max_bytes = FILE_HEAD + nd + FILE_REST;
    if (p.max_bytes > INT32_MAX || nb * H > INT32_MAX) return p;
    p.stream_stride = (int64_t)up16((size_t)nd + 4);
    const size_t stripes = (size_t)nb * (size_t)p.ns;
    p.codes_at = up16((size_t)nb * (size_t)H * (size_t)p.n1);
    p.hdr_at = p.codes_at + up16(stripes * CODE_LD * 4);
    p.hbits_at = p.hdr_at + stripes * HDR_WORDS * 4;
    p.sbits_at = p.hbits_at + up16(stripes * 4);
    p.cleared_at = p.sbits_at + up16(stripes * 8);
    p.stream_at = p.cleared_at + stripes * 256 * 4;
    p.bytes = p.stream_at + (size_t)nb * (size_t)p.stream_stride + 16;            // 16: the alignment of a workspace that arrives unaligned
    p.ok = true;
    return p;
}

}  // namespace

extern "C" size_t ideas_png_file_max_bytes(int C, int H, int W) {
    const png_plan p = plan_for(1, C, H, W);
    return p.ok ? (size_t)p.max_bytes : 0;
}

extern "C" size_t ideas_png_file_encode_workspace_bytes(int B, int C, int H, int W) {
    if (B <= 0) return 0;
    const png_plan p = plan_for(B, C, H, W);
    return p.ok ? p.bytes : 0;
}

extern "C" int ideas_png_file_encode(void* files, int* nbytes, long long row_stride, const void* u8, void* workspace, int B, int C, int H,
                                     int W, void* stream_) {
    if (!files || !nbytes || !u8 || !workspace) return IDEAS_E_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return IDEAS_E_SHAPE;
    if (C != 1 && C != 3) return IDEAS_E_UNSUPPORTED;
    const png_plan p = plan_for(B, C, H, W);
    if (!p.ok || row_stride < p.max_bytes) return IDEAS_E_SHAPE;
    hipStream_t stream = (hipStream_t)stream_;

    unsigned char* base = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(workspace) + 15) & ~(uintptr_t)15);
    unsigned char* filt = base;
    unsigned* codes = reinterpret_cast<unsigned*>(base + p.codes_at);
    unsigned* hdr = reinterpret_cast<unsigned*>(base + p.hdr_at);
    unsigned* hbits = reinterpret_cast<unsigned*>(base + p.hbits_at);
    uint64_t* sbits = reinterpret_cast<uint64_t*>(base + p.sbits_at);
    unsigned* hist = reinterpret_cast<unsigned*>(base + p.cleared_at);
    unsigned char* bits = base + p.stream_at;
    // the histograms and the words the bits are ORed into, in one stretch
    const hipError_t e = hipMemsetAsync(hist, 0, p.stream_at - p.cleared_at + (size_t)B * (size_t)p.stream_stride, stream);
    if (e != hipSuccess) return (int)e;

    const unsigned stripes = (unsigned)((int64_t)B * p.ns);
    hipLaunchKernelGGL(filter_kernel, dim3((unsigned)((int64_t)B * H)), dim3(256), 0, stream, filt, hist, (const unsigned char*)u8, H,
                       p.n1 - 1, C, p.ns);
    hipLaunchKernelGGL(tables_kernel, dim3(stripes), dim3(64), 0, stream, codes, hdr, hbits, sbits, (const unsigned*)hist, p.ns);
    hipLaunchKernelGGL(pack_kernel, dim3(stripes), dim3(256), 0, stream, (unsigned*)bits, p.stream_stride / 4, (const unsigned char*)filt,
                       (const unsigned*)codes, (const unsigned*)hdr, (const unsigned*)hbits, (const uint64_t*)sbits, H, p.n1, p.ns);
    hipLaunchKernelGGL(finish_kernel, dim3(B), dim3(FIN_THREADS), 0, stream, (unsigned char*)files, nbytes, (int64_t)row_stride,
                       (const unsigned char*)bits, p.stream_stride, (const unsigned char*)filt, (const uint64_t*)sbits, C, H, W, p.ns);
    return ideas_launch_status();
}
