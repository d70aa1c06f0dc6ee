// The bytes of the 8-bit container, said once for stego.hip, attack.hip, attack_spatial.hip and attack_jpeg.hip: what a reader makes of
// a byte, the clamp to a byte, a byte out of packed words, and the store of N consecutive bytes of `out` with their received values
// `y`.  Every kernel of the four files that writes the container writes it through store_bytes.  DESIGN.md 8.8.
#pragma once
#include "common.hpp"

namespace {

// The received value of a byte.  It must equal what ideas_image_u8_to_f32(mean 0.5, std 0.5) makes of it: csrc/image_io.hip's two
// steps, two true divisions, no contraction.
__device__ __forceinline__ float byte_to_unit(unsigned q) {
    float t;
    {
#pragma clang fp contract(off)
        t = (float)q / 255.0f;
        t = (t - 0.5f) / 0.5f;
    }
    return t;
}

// byte -> received f32 as a table in LDS: the two divisions once a workgroup (of 256 threads; the caller's barrier follows)
__device__ __forceinline__ void fill_unit(float (&s_unit)[256]) { s_unit[threadIdx.x] = byte_to_unit(threadIdx.x); }

// the two ways store_bytes comes by a received value
struct unit_direct {
    __device__ __forceinline__ float operator()(unsigned b) const { return byte_to_unit(b); }
};
struct unit_table {
    const float* s;                                          // fill_unit's table
    __device__ __forceinline__ float operator()(unsigned b) const { return s[b]; }
};

__device__ __forceinline__ int clamp_u8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// byte i (a compile-time index after unrolling) of consecutive little-endian words
template <int N> __device__ __forceinline__ unsigned byte_of(const unsigned (&w)[N], int i) { return (w[i >> 2] >> ((i & 3) * 8)) & 0xffu; }

__device__ __forceinline__ unsigned pack4(const unsigned* b) { return b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24); }

// N consecutive bytes b (each 0..255) at byte offset o of out, and their received values at y + o if y is given.
// WB = 4 or 8, the vector form: N / WB words of WB bytes, then N / 4 float4; out + o is WB-byte and y + o 16-byte aligned.
// WB = 0, the byte form: the first `nvalid` groups of G bytes (G = 1: bytes; G = C: whole pixels), one byte and one float at a time.
template <int N, int WB, int G = 1, class Unit>
__device__ __forceinline__ void store_bytes(unsigned char* __restrict__ out, float* __restrict__ y, int64_t o, const unsigned* b, int nvalid,
                                            Unit unit) {
    if constexpr (WB == 8) {
#pragma unroll
        for (int k = 0; k < N / 8; ++k) reinterpret_cast<uint2*>(out + o)[k] = make_uint2(pack4(b + 8 * k), pack4(b + 8 * k + 4));
    } else if constexpr (WB == 4) {
#pragma unroll
        for (int k = 0; k < N / 4; ++k) reinterpret_cast<unsigned*>(out + o)[k] = pack4(b + 4 * k);
    }
    if constexpr (WB != 0) {
        if (y) {
#pragma unroll
            for (int k = 0; k < N / 4; ++k)
                reinterpret_cast<float4*>(y + o)[k] = make_float4(unit(b[4 * k]), unit(b[4 * k + 1]), unit(b[4 * k + 2]), unit(b[4 * k + 3]));
        }
    } else {
#pragma unroll
        for (int g = 0; g < N / G; ++g) {
            if (g < nvalid) {
#pragma unroll
                for (int e = g * G; e < (g + 1) * G; ++e) {
                    out[o + e] = (unsigned char)b[e];
                    if (y) y[o + e] = unit(b[e]);
                }
            }
        }
    }
}

}  // namespace
