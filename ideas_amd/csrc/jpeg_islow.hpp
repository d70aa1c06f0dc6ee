// The decoding half of the libjpeg-exact integer model, shared by the round trip (attack_jpeg.hip) and the file reader
// (jpeg_decode.hip): the constants of the "islow" 8-point transform, its odd part, the inverse pass, and the triangle chroma upsampler
// of 4:2:0 (a macro: see there).  The model is stated step by step in include/ideas_hip.h ("The JPEG file channel", steps 7 and 8).
#pragma once
#include "jpeg_block.hpp"

namespace {

// round(c * 2^13) of the twelve constants of the 8-point transform
constexpr int F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633;
constexpr int F_1_501 = 12299, F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;
constexpr int CONST_BITS = 13, PASS1_BITS = 2;

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// The odd half both transforms share: (t4, t5, t6, t7) -> four rotated sums.  Every factor stays below 2^23 and every product below
// 2^31 for what an encoder produces (tests/jpegfile_ref.py asserts it on every product), so the 24-bit multiply is exact.
__device__ __forceinline__ void odd_part(int t4, int t5, int t6, int t7, int& a4, int& a5, int& a6, int& a7) {
    const int z5 = __mul24(t4 + t6 + t5 + t7, F_1_175);
    const int z1 = __mul24(t4 + t7, -F_0_899), z2 = __mul24(t5 + t6, -F_2_562);
    const int z3 = __mul24(t4 + t6, -F_1_961) + z5, z4 = __mul24(t5 + t7, -F_0_390) + z5;
    a4 = __mul24(t4, F_0_298) + z1 + z3;
    a5 = __mul24(t5, F_2_053) + z2 + z4;
    a6 = __mul24(t6, F_3_072) + z2 + z3;
    a7 = __mul24(t7, F_1_501) + z1 + z4;
}

// FIRST: the column pass (DESCALE by 11); otherwise the row pass (by 18)
template <bool FIRST> __device__ __forceinline__ void idct_pass(const int (&c)[8], int (&o)[8]) {
    const int z1 = __mul24(c[2] + c[6], F_0_541);
    const int t2 = z1 + __mul24(c[6], -F_1_847), t3 = z1 + __mul24(c[2], F_0_765);
    const int t0 = (c[0] + c[4]) << CONST_BITS, t1 = (c[0] - c[4]) << CONST_BITS;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int a0, a1, a2, a3;
    odd_part(c[7], c[5], c[3], c[1], a0, a1, a2, a3);
    constexpr int N = FIRST ? CONST_BITS - PASS1_BITS : CONST_BITS + PASS1_BITS + 3;
    o[0] = descale(t10 + a3, N); o[7] = descale(t10 - a3, N);
    o[1] = descale(t11 + a2, N); o[6] = descale(t11 - a2, N);
    o[2] = descale(t12 + a1, N); o[5] = descale(t12 - a1, N);
    o[3] = descale(t13 + a0, N); o[4] = descale(t13 - a0, N);
}

// Chroma up at 4:2:0 for the lane that owns pixels 8 bx .. 8 bx + 7 of image row yy: pl[1], pl[2] = Cb, Cr from half, uint8
// [B][2][ch][cw], b the image.  The triangle filter on the REAL ch x cw samples, neighbours clamped to them: s = 3 c(i, .) + c(i', .),
// i' the row above for an even output row and the one below for an odd one; columns 4 bx - 1 .. 4 bx + 4 serve the lane's 8 pixels.
// A macro and not a function: as a function, however its arguments are cut, the round trip's jpeg_file_kernel<3, 2, *> compiles to 5 %
// more instructions and 15 more VGPRs (one wave per SIMD fewer) than with these lines in its body; as text it compiles to the same
// instructions as before (tools/isa_diff.py).
#define IDEAS_UPSAMPLE420_ROW(half, b, H, W, yy, bx, pl)                                                                            \
    {                                                                                                                               \
        const int ch = ((H) + 1) >> 1, cw = ((W) + 1) >> 1;                                                                         \
        const int yc = (yy) < (H) ? (yy) : (H) - 1;                                                                                 \
        const int i = yc >> 1;                                                                                                      \
        const int i2 = (yc & 1) ? (i + 1 < ch ? i + 1 : ch - 1) : (i > 0 ? i - 1 : 0);                                              \
        const bool plain = cw <= 2; /* W <= 4: the library copies every chroma sample to its 2x2 pixels */                          \
        _Pragma("unroll") for (int p = 0; p < 2; ++p) {                                                                             \
            const unsigned char* c0 = (half) + (((b) * 2 + p) * ch + i) * cw;                                                       \
            const unsigned char* c1 = (half) + (((b) * 2 + p) * ch + i2) * cw;                                                      \
            int s[6], c[6];                                                                                                         \
            _Pragma("unroll") for (int k = 0; k < 6; ++k) {                                                                         \
                int j = 4 * (bx) - 1 + k;                                                                                           \
                j = j < 0 ? 0 : (j > cw - 1 ? cw - 1 : j);                                                                          \
                c[k] = c0[j];                                                                                                       \
                s[k] = 3 * c[k] + (int)c1[j];                                                                                       \
            }                                                                                                                       \
            _Pragma("unroll") for (int k = 0; k < 4; ++k) {                                                                         \
                (pl)[1 + p][2 * k] = plain ? c[k + 1] : (3 * s[k + 1] + s[k] + 8) >> 4;                                             \
                (pl)[1 + p][2 * k + 1] = plain ? c[k + 1] : (3 * s[k + 1] + s[k + 2] + 7) >> 4;                                     \
            }                                                                                                                       \
        }                                                                                                                           \
    }

}  // namespace
