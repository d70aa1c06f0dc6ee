// Payload coding, device side: a rate-compatible punctured convolutional code (K = 7, generators 171 / 133 octal, rates 1/2, 2/3,
// 3/4), an interleaver over each image, the soft demapper of the extractor's output and a soft-decision Viterbi decoder.  Every image
// is one zero-terminated codeword.  The code is defined step by step in include/ideas_hip.h ("Payload coding") and DESIGN.md, and
// restated in numpy by tests/ecc_ref.py; the decoder is integer arithmetic with a fixed tie rule, so all three agree to the bit.
//
// Viterbi: one wave per image, lane = trellis state (64 states, 64 lanes).  Per chunk of 64 steps lane j gathers the two soft values
// of step t0 + j (de-interleaved, punctured positions 0) and the values of the next chunk are in flight while this one runs.  Per step
// the two soft values come out of lane j by v_readlane, the two predecessor metrics by cross-lane reads, and the 64 decisions are one
// __ballot; lane j keeps the word of step t0 + j, so a chunk's survivors leave as one 512-byte store.  The traceback reads them back the
// same way and walks a chunk in scalar registers.
#include "stream.hpp"

namespace {

constexpr unsigned G0 = 0171, G1 = 0133;                     // on r_t = (u_t << 6) | (r_{t-1} >> 1): u_t in bit 6, u_{t-6} in bit 0
constexpr int TAIL = 6;
constexpr int MAX_STEPS = 1 << 20;                           // 254 * 2^20 + 2^30 < 2^31: int32 metrics need no normalisation
constexpr int LDS_CAP = 32768;                               // bytes of survivors (8 a step) a wave keeps in LDS: T <= 4096
constexpr int CHUNK = 64;

constexpr unsigned rev7(unsigned g) {
    unsigned r = 0;
    for (int i = 0; i < 7; ++i) r |= ((g >> i) & 1u) << (6 - i);
    return r;
}

// Puncturing as ONE bit pattern a period: bit 2 r + o says that output o (0: c0, 1: c1) of a step with t % period == r is kept.  The
// kept outputs are numbered in the order of those bits.
struct Punct {
    int period, kept;
    unsigned pat;
};
__host__ __device__ inline Punct punct_of(int rate) {
    switch (rate) {
        case IDEAS_ECC_RATE_2_3: return Punct{2, 3, 0x07u};  // c0: 1 1, c1: 1 0
        case IDEAS_ECC_RATE_3_4: return Punct{3, 4, 0x27u};  // c0: 1 1 0, c1: 1 0 1
        default: return Punct{1, 2, 0x03u};
    }
}
// kept outputs of the steps before t: m(t)
__host__ __device__ inline int64_t kept_before(const Punct& p, int64_t t) {
    const int64_t a = t / p.period;
    const int r = (int)(t - a * p.period);
    return a * p.kept + __builtin_popcount(p.pat & ((1u << (2 * r)) - 1u));
}

int64_t gcd64(int64_t a, int64_t b) {
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// what encoder and decoder check alike; T = k + 6
int check_code(int B, int n, int k, int rate, int P) {
    if (B <= 0 || n <= 0 || k <= 0) return IDEAS_E_SHAPE;
    if (rate != IDEAS_ECC_RATE_1_2 && rate != IDEAS_ECC_RATE_2_3 && rate != IDEAS_ECC_RATE_3_4) return IDEAS_E_UNSUPPORTED;
    if (k % 8 != 0 || (int64_t)k + TAIL > MAX_STEPS) return IDEAS_E_SHAPE;
    if (kept_before(punct_of(rate), (int64_t)k + TAIL) > n) return IDEAS_E_SHAPE;
    if (P < 1 || P >= n || gcd64(P, n) != 1) return IDEAS_E_SHAPE;
    return IDEAS_OK;
}

// ---- encoder ---------------------------------------------------------------------------------------------------------------------
// A thread owns bytes of the coded rows.  Message bit j carries coded position i = (j * Pinv) mod n: one 64-bit product a byte, then
// i += Pinv (mod n) from bit to bit.  i < m: the parity of the 7-bit window of the info row behind kept output i; else the fill bit.
__global__ __launch_bounds__(256) void ecc_encode_kernel(unsigned char* __restrict__ coded, const unsigned char* __restrict__ info,
                                                         const unsigned char* __restrict__ fill, int64_t total, int n, int k, int rate,
                                                         unsigned Pinv, int64_t nbytes, int m) {
    const Punct pu = punct_of(rate);
    const int kbytes = k >> 3;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int64_t b = idx / nbytes;
        const int64_t kb = idx - b * nbytes;
        const unsigned char* row = info + b * kbytes;
        const unsigned fbyte = fill ? fill[idx] : 0u;
        unsigned i = (unsigned)(((uint64_t)(kb * 8) * Pinv) % (unsigned)n);
        unsigned byte = 0;
        for (int bit = 0; bit < 8 && kb * 8 + bit < n; ++bit) {
            unsigned v;
            if ((int)i < m) {
                const unsigned a = i / (unsigned)pu.kept;
                int rem = (int)(i - a * pu.kept), pos = 0;
                for (;; ++pos) {                              // the rem-th set bit of the pattern
                    if ((pu.pat >> pos) & 1u) {
                        if (rem == 0) break;
                        --rem;
                    }
                }
                const int t = (int)a * pu.period + (pos >> 1);
                // info bits t - 6 .. t, oldest in bit 6 (the packed rows are most significant bit first): at most two bytes, and a
                // byte outside the row is zero -- the register before the first bit and the six terminating steps
                const int xs = t - TAIL + 8;
                const int k0 = (xs >> 3) - 1;
                const unsigned hi = k0 >= 0 && k0 < kbytes ? row[k0] : 0u;
                const unsigned lo = k0 + 1 < kbytes ? row[k0 + 1] : 0u;
                const unsigned win = (((hi << 8) | lo) >> (9 - (xs & 7))) & 0x7fu;
                v = (unsigned)__popc(win & ((pos & 1) ? rev7(G1) : rev7(G0))) & 1u;
            } else {
                v = (fbyte >> (7 - bit)) & 1u;
            }
            byte |= v << (7 - bit);
            i += Pinv;
            if (i >= (unsigned)n) i -= (unsigned)n;
        }
        coded[idx] = (unsigned char)byte;
    }
}

// ---- soft demapper ---------------------------------------------------------------------------------------------------------------
// A thread owns one message bit: the squared distances of the clamped element to every bin centre, the nearest with the bit 0 and the
// nearest with the bit 1.  Every step is one f32 operation in the header's order.
template <typename T>
__global__ __launch_bounds__(256) void ecc_soft_kernel(signed char* __restrict__ soft, const T* __restrict__ z, int64_t total, int sigma,
                                                       float step, float step2, float gain) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int nbin = 1 << sigma;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int64_t e = idx / sigma;
        const int sh = sigma - 1 - (int)(idx - e * sigma);
        const float zv = ld1(z + e);
        float r;
        {
#pragma clang fp contract(off)
            const float c = fminf(fmaxf(zv, -1.0f), 1.0f);   // a NaN comes out as -1, as in stego.hip's decode1
            float d0 = INFINITY, d1 = INFINITY;
            for (int v = 0; v < nbin; ++v) {
                const float cv = step * ((float)v + 0.5f) - 1.0f;      // exact: a multiple of 2^-8 in (-1, 1)
                float d = c - cv;
                d = d * d;
                if ((v >> sh) & 1) d1 = fminf(d1, d); else d0 = fminf(d0, d);
            }
            float t = d0 - d1;
            t = t / step2;
            t = t * gain;
            r = fminf(fmaxf(rintf(t), -127.0f), 127.0f);
        }
        soft[idx] = (signed char)(int)r;
    }
}

// ---- decoder ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int bcast(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }      // lane: wave-uniform

template <bool GLOBAL>
__global__ __launch_bounds__(64) void ecc_viterbi_kernel(unsigned char* __restrict__ info, int* __restrict__ metric,
                                                         const signed char* __restrict__ soft, unsigned long long* __restrict__ workspace,
                                                         int n, int k, int rate, unsigned P) {
    extern __shared__ unsigned long long s_surv[];
    const int lane = (int)threadIdx.x;
    const int64_t b = blockIdx.x;
    const int T = k + TAIL;
    const signed char* q = soft + b * n;
    unsigned long long* surv = GLOBAL ? workspace + b * T : s_surv;
    const Punct pu = punct_of(rate);
    const bool small = (unsigned)n <= 65536u;                // i * P < 2^32: the position without a 64-bit division

    // the outputs of the two transitions into state `lane`: r = (lane << 1) | b, as signs on (q of c0, q of c1)
    const unsigned ra = (unsigned)lane << 1, rb = ra | 1u;
    const int a0 = (__popc(ra & G0) & 1) ? 1 : -1, a1 = (__popc(ra & G1) & 1) ? 1 : -1;
    const int b0 = (__popc(rb & G0) & 1) ? 1 : -1, b1 = (__popc(rb & G1) & 1) ? 1 : -1;
    const int p0 = (lane & 31) << 1, p1 = p0 | 1;

    // the soft values of step t: a punctured output and a step past the end count 0
    auto gather = [&](int t, int& q0, int& q1) {
        q0 = q1 = 0;
        if (t >= T) return;
        const unsigned a = (unsigned)t / (unsigned)pu.period;
        const int r2 = 2 * (t - (int)a * pu.period);
        unsigned i = a * pu.kept + __popc(pu.pat & ((1u << r2) - 1u));
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            if ((pu.pat >> (r2 + o)) & 1u) {
                const unsigned pos = small ? (i * P) % (unsigned)n : (unsigned)(((uint64_t)i * P) % (unsigned)n);
                const int v = q[pos];
                if (o == 0) q0 = v; else q1 = v;
                ++i;
            }
        }
    };

    int pm = lane == 0 ? 0 : -(1 << 30);
    int nq0, nq1;
    gather(lane, nq0, nq1);
    for (int t0 = 0; t0 < T; t0 += CHUNK) {
        const int q0v = nq0, q1v = nq1;
        if (t0 + CHUNK < T) gather(t0 + CHUNK + lane, nq0, nq1);
        const int cnt = T - t0 < CHUNK ? T - t0 : CHUNK;
        unsigned long long word = 0;
        auto acs = [&](int j) {
            const int q0 = bcast(q0v, j), q1 = bcast(q1v, j);
            const int ma = __shfl(pm, p0, 64) + (a0 * q0 + a1 * q1);
            const int mb = __shfl(pm, p1, 64) + (b0 * q0 + b1 * q1);
            const bool dec = mb > ma;                        // equal metrics: b = 0 wins
            pm = dec ? mb : ma;
            const unsigned long long bal = __ballot(dec);
            if (lane == j) word = bal;
        };
        if (cnt == CHUNK) {
#pragma unroll 16
            for (int j = 0; j < CHUNK; ++j) acs(j);
        } else {
            for (int j = 0; j < cnt; ++j) acs(j);
        }
        if (lane < cnt) surv[t0 + lane] = word;
    }
    if (metric && lane == 0) metric[b] = pm;
    if (GLOBAL) __threadfence();                             // the words other lanes stored are read below
    __syncthreads();

    // traceback from state 0: u_t is bit 5 of the state after step t, the survivor bit leads to the state before it
    const int kbytes = k >> 3;
    int s = 0;
    for (int t0 = ((T - 1) / CHUNK) * CHUNK; t0 >= 0; t0 -= CHUNK) {
        const int cnt = T - t0 < CHUNK ? T - t0 : CHUNK;
        const unsigned long long w = lane < cnt ? surv[t0 + lane] : 0ull;
        const int wlo = (int)(unsigned)w, whi = (int)(unsigned)(w >> 32);
        unsigned long long bits = 0;
        for (int j = cnt - 1; j >= 0; --j) {
            const unsigned half = (unsigned)(s < 32 ? bcast(wlo, j) : bcast(whi, j));
            bits |= (unsigned long long)(s >> 5) << j;
            s = ((s & 31) << 1) | (int)((half >> (s & 31)) & 1u);
        }
        if (lane < 8 && t0 + 8 * lane < k)                   // whole bytes of the info row only: k % 8 == 0, the tail is dropped
            info[b * kbytes + (t0 >> 3) + lane] = (unsigned char)(__brev((unsigned)(bits >> (8 * lane)) & 0xffu) >> 24);
    }
}

unsigned flat_grid(int64_t threads) {
    int64_t grid = ideas_cdiv(threads, 256);
    if (grid > 16384) grid = 16384;
    return (unsigned)(grid < 1 ? 1 : grid);
}

}  // namespace

extern "C" int ideas_ecc_encode(void* coded, const void* info, const void* fill, int B, int n, int k, int rate, int P, int Pinv,
                                void* stream_) {
    if (!coded || !info) return IDEAS_E_NULL;
    const int rc = check_code(B, n, k, rate, P);
    if (rc != IDEAS_OK) return rc;
    if (Pinv < 1 || Pinv >= n || ((int64_t)P * Pinv) % n != 1) return IDEAS_E_SHAPE;
    const int64_t nbytes = ((int64_t)n + 7) / 8, total = nbytes * B;
    const int m = (int)kept_before(punct_of(rate), (int64_t)k + TAIL);
    hipLaunchKernelGGL(ecc_encode_kernel, dim3(flat_grid(total)), dim3(256), 0, (hipStream_t)stream_, (unsigned char*)coded,
                       (const unsigned char*)info, (const unsigned char*)fill, total, n, k, rate, (unsigned)Pinv, nbytes, m);
    return ideas_launch_status();
}

extern "C" int ideas_ecc_soft(void* soft, const void* z, int B, int L, int sigma, float gain, int dtype, void* stream_) {
    if (!soft || !z) return IDEAS_E_NULL;
    if (B <= 0 || L <= 0) return IDEAS_E_SHAPE;
    if (sigma < 1 || sigma > 8) return IDEAS_E_UNSUPPORTED;
    if (dtype != IDEAS_F32 && dtype != IDEAS_BF16) return IDEAS_E_UNSUPPORTED;
    if (!(gain > 0.0f) || gain > 3.0e38f) return IDEAS_E_UNSUPPORTED;      // positive and finite
    const float step = 2.0f / (float)(1 << sigma);
    const int64_t total = (int64_t)B * L * sigma;
    hipStream_t stream = (hipStream_t)stream_;
    with_dtype(dtype, [&](auto c) {
        using T = typename decltype(c)::type;
        hipLaunchKernelGGL(ecc_soft_kernel<T>, dim3(flat_grid(total)), dim3(256), 0, stream, (signed char*)soft, (const T*)z, total, sigma,
                           step, step * step, gain);
        return 0;
    });
    return ideas_launch_status();
}

extern "C" int ideas_ecc_viterbi(void* info, int* metric, const void* soft, void* workspace, int B, int n, int k, int rate, int P,
                                 void* stream_) {
    if (!info || !soft) return IDEAS_E_NULL;
    const int rc = check_code(B, n, k, rate, P);
    if (rc != IDEAS_OK) return rc;
    const int T = k + TAIL;
    if (!workspace && 8 * (int64_t)T > LDS_CAP) return IDEAS_E_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    if (workspace)
        hipLaunchKernelGGL(ecc_viterbi_kernel<true>, dim3((unsigned)B), dim3(64), 0, stream, (unsigned char*)info, metric,
                           (const signed char*)soft, (unsigned long long*)workspace, n, k, rate, (unsigned)P);
    else
        hipLaunchKernelGGL(ecc_viterbi_kernel<false>, dim3((unsigned)B), dim3(64), (size_t)(8 * T), stream, (unsigned char*)info, metric,
                           (const signed char*)soft, (unsigned long long*)nullptr, n, k, rate, (unsigned)P);
    return ideas_launch_status();
}
