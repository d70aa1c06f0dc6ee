// What the HBM-bound "streaming" kernels share: channel-vector I/O, the fixed-order sums, the vector-width and lane-group rules and
// the dispatch from the run-time (dtype, vector width) to a <T, VW> instantiation.  DESIGN.md §3.1.2 lists which source uses what.
//
// Tensors are channels-innermost in f32 or bf16, arithmetic is f32, one rounding at the store.  A pixel's C channels are moved as
// 16-byte vectors of VW elements (4 f32 / 8 bf16) when C % VW == 0 and every pointer is 16-byte aligned, and element by element
// (VW = 1: any C, any element-aligned pointer) otherwise.
#pragma once
#include <type_traits>
#include "common.hpp"

// ---- device --------------------------------------------------------------------------------------------------------------------
// VW consecutive elements <-> f32: one 16-byte access for (float, 4) and (bf16, 8), an element access for VW = 1
template <typename T, int VW> struct chan_io;
template <typename T> struct chan_io<T, 1> {
    static __device__ __forceinline__ void load(const T* p, float (&f)[1]) { f[0] = ld1(p); }
    static __device__ __forceinline__ void store(T* p, const float (&f)[1]) { st1(p, f[0]); }
};
template <> struct chan_io<float, 4> {
    static __device__ __forceinline__ void load(const float* p, float (&f)[4]) {
        const float4 v = *reinterpret_cast<const float4*>(p);
        f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
    }
    static __device__ __forceinline__ void store(float* p, const float (&f)[4]) {
        *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
    }
};
template <> struct chan_io<ideas_bf16, 8> {
    static __device__ __forceinline__ void load(const ideas_bf16* p, float (&f)[8]) {
        unpack8(*reinterpret_cast<const uint4*>(p), f, ideas_bf16{});
    }
    static __device__ __forceinline__ void store(ideas_bf16* p, const float (&f)[8]) {
        *reinterpret_cast<uint4*>(p) = pack8(f, ideas_bf16{});
    }
};

// VW consecutive f32 side values (a bias): 16-byte loads on the vector paths (the host checked the alignment)
template <int VW>
__device__ __forceinline__ void load_f32(const float* p, float (&f)[VW]) {
    if constexpr (VW == 1) {
        f[0] = p[0];
    } else {
#pragma unroll
        for (int q = 0; q < VW; q += 4) {
            const float4 v = *reinterpret_cast<const float4*>(p + q);
            f[q] = v.x; f[q + 1] = v.y; f[q + 2] = v.z; f[q + 3] = v.w;
        }
    }
}

// the sum over the G lanes of a group (G a power of two <= 64), the same value in each of them; every lane of the wave calls it
__device__ __forceinline__ float group_sum(float v, int G) {
    for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sum over a block of 256 threads with a fixed association: the xor butterfly in each wave, then ((s0 + s1) + s2) + s3 over the
// four waves; the result is valid in EVERY thread.  FIRST_USE: nothing has read s_part since the block's last barrier (a kernel
// that calls it once), so the barrier in front of the write is left out.
template <typename S, bool FIRST_USE = false>
__device__ __forceinline__ S block_sum_256(S v, S* s_part) {
    v = wave_sum(v);
    if constexpr (!FIRST_USE) __syncthreads();            // s_part may still be read from a previous call
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// elements of a channel vector: 8 (bf16) or 4 (f32) when the pointers are 16-byte aligned and C is a multiple of it, else 1
static inline int ideas_chan_vw(int dtype, int C, bool aligned) {
    const int w = dtype == IDEAS_BF16 ? 8 : 4;
    return (aligned && C % w == 0) ? w : 1;
}
// lanes that own a pixel of L vectors: the power of two >= min(L, 64); it divides 64, so a group never straddles a wave
static inline int ideas_lane_group(int L) {
    int G = 1;
    while (G < L && G < 64) G <<= 1;
    return G;
}

// storage type and vector width as a value: what with_chan / with_dtype hand to their visitor
template <typename T, int VW_ = 1> struct chan {
    typedef T type;
    static constexpr int VW = VW_;
};
// f(chan<T, VW>{}) for the dtype (checked by the caller: IDEAS_F32 or IDEAS_BF16) and the width ideas_chan_vw chose
template <typename F> static inline void with_chan(int dtype, int vw, F&& f) {
    if (dtype == IDEAS_BF16) { if (vw == 8) f(chan<ideas_bf16, 8>{}); else f(chan<ideas_bf16, 1>{}); }
    else { if (vw == 4) f(chan<float, 4>{}); else f(chan<float, 1>{}); }
}
// f(chan<T>{}) for the dtype alone; returns what f returns
template <typename F> static inline auto with_dtype(int dtype, F&& f) {
    return dtype == IDEAS_BF16 ? f(chan<ideas_bf16>{}) : f(chan<float>{});
}
