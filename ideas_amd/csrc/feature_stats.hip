// Streaming first and second moments of a feature matrix in f64 (the statistics of the Frechet Inception distance,
// stylegan2/fid.py:97-98 and calc_inception.py:110-111 without keeping the features):
//
//     sum[d]     += sum_n x[n][d]                  gram[i][j] += sum_n x[n][i] x[n][j]            x float [N][D], sum / gram double
//
// Every product and every sum is f64 (the f32 features widen exactly).  One thread owns an output element from its load to its
// store and adds the N terms to the value already there in index order, n = 0 .. N-1, with one fused multiply-add each: no atomics,
// no split over n, so two runs are bitwise equal and updating with two batches is bitwise the update with their concatenation.
// gram[i][j] and gram[j][i] run the same sequence of operations on the same (commutative) products: the full D x D matrix is
// written and is symmetric by construction, nothing is mirrored afterwards.
//
// Layout: a workgroup of 256 threads owns a 64 x 64 tile of gram; thread (ty, tx) = (t / 16, t % 16) owns the 4 x 4 elements
// (ty + 16 a, tx + 16 b): consecutive tx are consecutive columns, so the tile's loads and stores are 128-byte runs.  The rows of x
// pass through LDS in chunks of FS_NK: xi[k][0..64) = the tile's row features, xj[k][0..64) = its column features, widened to
// double on the way in (2 x 16 x 64 x 8 B = 16 KiB); per k a thread reads 4 + 4 doubles (the xi reads are broadcasts within a
// quarter wave, the xj reads consecutive) for 16 FMAs.  Columns past D are loaded as zeros and never stored.  The hot shape
// (N = 64, D = 2048, once per batch of the FID loop) is 0.5 GFLOP against 64 MiB of gram traffic: the kernel is bound by reading
// and writing gram, not by the f64 VALU rate, which is why the plain tiled form is kept.
#include "common.hpp"

namespace {

constexpr int FS_T = 64;          // tile edge
constexpr int FS_NK = 16;         // rows of x per LDS chunk

__global__ __launch_bounds__(256) void feature_gram_kernel(double* __restrict__ gram, const float* __restrict__ x, int N, int D) {
    __shared__ double xi[FS_NK][FS_T];
    __shared__ double xj[FS_NK][FS_T];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int i0 = blockIdx.y * FS_T, j0 = blockIdx.x * FS_T;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
            acc[a][b] = (i < D && j < D) ? gram[(int64_t)i * D + j] : 0.0;
        }
    for (int n0 = 0; n0 < N; n0 += FS_NK) {
        // 2 x FS_NK x FS_T = 2048 elements, 8 per thread; consecutive threads read consecutive features of one row of x
#pragma unroll
        for (int q = 0; q < (FS_NK * FS_T) / 256; ++q) {
            const int e = q * 256 + t, k = e / FS_T, c = e % FS_T;
            const int n = n0 + k;
            const bool row = n < N;
            xi[k][c] = (row && i0 + c < D) ? (double)x[(int64_t)n * D + i0 + c] : 0.0;
            xj[k][c] = (row && j0 + c < D) ? (double)x[(int64_t)n * D + j0 + c] : 0.0;
        }
        __syncthreads();
        const int kn = N - n0 < FS_NK ? N - n0 : FS_NK;          // (rows past N are zeros, but adding +0 products is skipped anyway)
        for (int k = 0; k < kn; ++k) {
            double vi[4], vj[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) vi[a] = xi[k][ty + 16 * a];
#pragma unroll
            for (int b = 0; b < 4; ++b) vj[b] = xj[k][tx + 16 * b];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = fma(vi[a], vj[b], acc[a][b]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
            if (i < D && j < D) gram[(int64_t)i * D + j] = acc[a][b];
        }
}

// one thread per feature: the N rows in index order
__global__ __launch_bounds__(256) void feature_sum_kernel(double* __restrict__ sum, const float* __restrict__ x, int N, int D) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= D) return;
    double s = sum[d];
    for (int n = 0; n < N; ++n) s += (double)x[(int64_t)n * D + d];
    sum[d] = s;
}

}  // namespace

extern "C" int ideas_feature_stats_accum(double* sum, double* gram, const float* x, int N, int D, void* stream_) {
    if (N <= 0 || D <= 0) return IDEAS_E_SHAPE;
    if (D > IDEAS_FEATURE_STATS_MAX_DIM) return IDEAS_E_UNSUPPORTED;
    if (!sum || !gram || !x) return IDEAS_E_NULL;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(feature_sum_kernel, dim3((unsigned)ideas_cdiv(D, 256)), dim3(256), 0, stream, sum, x, N, D);
    const int st = ideas_launch_status();
    if (st) return st;
    const unsigned tiles = (unsigned)ideas_cdiv(D, FS_T);
    hipLaunchKernelGGL(feature_gram_kernel, dim3(tiles, tiles), dim3(256), 0, stream, gram, x, N, D);
    return ideas_launch_status();
}
