// libjsgx.so, the 64 x 64 tile of pairwise costs that "cdist_64x64" (jsgx_cdist.hip) stores and "knn_64" (jsgx_knn.hip) selects from: one
// function, so the two kernels give the same bits.
//
// A GEMM-shaped N x M x K loop whose order of accumulation the header states (k ascending, one fmaf chain per output), so it runs
// on the vector pipe.  A workgroup of 256 lanes computes 64 x 64 costs of one pair; lane (ti, tj) = (tid / 16, tid % 16) holds the
// 4 x 4 outputs of rows 4 ti .. 4 ti + 3 and columns 4 tj .. 4 tj + 3 in registers.  Per panel of 32 features:
//   xs[k][f], ys[k][f]   64 frames of x and of y, feature-major with a row pitch of 68 words: the global reads run along k (the
//                        frame-major layout: 128 contiguous bytes per frame), a lane's four frames of one feature are one 16-byte
//                        LDS read; the 16 tj of a wavefront read 64 consecutive words of ys, its 4 ti are broadcasts of xs
// Frames past N or M are staged as zeros; a last panel shorter than 32 shortens the loop (uniformly), it adds no terms.
#pragma once

#include "jsgx_internal.h"

namespace jsgx {

constexpr int kTile = 64, kPanel = 32, kPitch = kTile + 4, kTileThreads = (kTile / 4) * (kTile / 4);
static_assert(JSGX_CDIST_TILE == kTile && JSGX_KNN_TILE == kTile && JSGX_KNN_STRIP == kTile, "include/jsgx.h states the tile");
static_assert(JSGX_CDIST_THREADS == kTileThreads && JSGX_KNN_THREADS == kTileThreads, "a lane holds 4 x 4 costs of the tile");
static_assert(2 * kPanel * kPitch * 4 == JSGX_CDIST_LDS_BYTES, "include/jsgx.h states the LDS");

// The two sequences of one pair and the two panels of LDS, kPanel * kPitch words each and 16-byte aligned.
struct CostTileArgs {
    const float* x;
    long long x_frame_pitch;
    const float* y;
    long long y_frame_pitch;
    int n, m, K;
    float* xs;
    float* ys;
};

struct CostTile {
    float c[4][4];      // [r][c]: row i0 + 4 ti + r, column j0 + 4 tj + c
};

// The finished costs of the tile at (i0, j0) that this lane holds.  Every lane of the workgroup calls it; the panels are free again
// behind the caller's next barrier.
template <int METRIC>
__device__ __forceinline__ CostTile cost_tile(const CostTileArgs& a, int i0, int j0) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    float acc[4][4], nx[4], ny[4];
    for (int r = 0; r < 4; ++r) {
        nx[r] = ny[r] = 0.f;
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
    }
    const int kk = tid & 31, f0 = tid >> 5;
    for (int k0 = 0; k0 < a.K; k0 += kPanel) {
        const int kc = a.K - k0 < kPanel ? a.K - k0 : kPanel;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int f = f0 + 8 * r;
            const bool k_in = kk < kc;
            a.xs[kk * kPitch + f] = (k_in && i0 + f < a.n) ? a.x[(long long)(i0 + f) * a.x_frame_pitch + k0 + kk] : 0.f;
            a.ys[kk * kPitch + f] = (k_in && j0 + f < a.m) ? a.y[(long long)(j0 + f) * a.y_frame_pitch + k0 + kk] : 0.f;
        }
        __syncthreads();
        for (int k = 0; k < kc; ++k) {
            const float4 xq = *reinterpret_cast<const float4*>(&a.xs[k * kPitch + 4 * ti]);
            const float4 yq = *reinterpret_cast<const float4*>(&a.ys[k * kPitch + 4 * tj]);
            const float xv[4] = {xq.x, xq.y, xq.z, xq.w}, yv[4] = {yq.x, yq.y, yq.z, yq.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (METRIC == JSGX_METRIC_COSINE) {
                        acc[r][c] = __builtin_fmaf(xv[r], yv[c], acc[r][c]);
                    } else {
                        const float d = xv[r] - yv[c];
                        acc[r][c] = __builtin_fmaf(d, d, acc[r][c]);
                    }
                }
            }
            if (METRIC == JSGX_METRIC_COSINE) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    nx[r] = __builtin_fmaf(xv[r], xv[r], nx[r]);
                    ny[r] = __builtin_fmaf(yv[r], yv[r], ny[r]);
                }
            }
        }
    }
    CostTile t;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (METRIC == JSGX_METRIC_SQEUCLIDEAN) {
                t.c[r][c] = acc[r][c];
            } else if (METRIC == JSGX_METRIC_EUCLIDEAN) {
                t.c[r][c] = sqrtf(acc[r][c]);
            } else {
                const float den = sqrtf(nx[r]) * sqrtf(ny[c]);
                t.c[r][c] = den == 0.f ? 1.0f : 1.0f - acc[r][c] / den;
            }
        }
    }
    return t;
}

}  // namespace jsgx
