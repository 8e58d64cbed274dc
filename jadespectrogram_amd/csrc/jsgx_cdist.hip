// libjsgx.so, the pairwise cost of two feature sequences (include/jsgx.h section 2): the kernel and its launcher.  The refusals and the
// plan are in jsgx_dtw_host.cpp.
//
// A GEMM-shaped N x M x K loop whose order of accumulation the header states (k ascending, one fmaf chain per output), so it runs
// on the vector pipe.  A workgroup of 256 lanes computes 64 x 64 costs of one pair; lane (ti, tj) = (tid / 16, tid % 16) holds the
// 4 x 4 outputs of rows 4 ti .. 4 ti + 3 and columns 4 tj .. 4 tj + 3 in registers.  Per panel of 32 features:
//   xs[k][f], ys[k][f]   64 frames of x and of y, feature-major with a row pitch of 68 words: the global reads run along k (the
//                        frame-major layout: 128 contiguous bytes per frame), a lane's four frames of one feature are one 16-byte
//                        LDS read; the 16 tj of a wavefront read 64 consecutive words of ys, its 4 ti are broadcasts of xs
// Frames past N or M are staged as zeros and never stored; a last panel shorter than 32 shortens the loop (uniformly), it adds no
// terms.  A row of the tile goes out as 16 lanes x 16 bytes = one 256-byte line (as 16-byte stores where cost is so aligned).
#include <hip/hip_runtime.h>

#include "jsgx_internal.h"

namespace jsgx {

struct CdistArgs {
    const float* x;
    long long x_frame_pitch, x_pair_pitch;
    const float* y;
    long long y_frame_pitch, y_pair_pitch;
    float* cost;
    long long cost_pitch, cost_pair_pitch;
    int n, m, K, vec;
};

constexpr int kTile = JSGX_CDIST_TILE, kPanel = 32, kPitch = kTile + 4;
static_assert(2 * kPanel * kPitch * 4 == JSGX_CDIST_LDS_BYTES, "include/jsgx.h states the LDS");

template <int METRIC>
__global__ __launch_bounds__(JSGX_CDIST_THREADS) void cdist_kernel(CdistArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float xs[kPanel * kPitch];
    __shared__ __attribute__((aligned(16))) float ys[kPanel * kPitch];
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
    const float* x = a.x + blockIdx.z * a.x_pair_pitch;
    const float* y = a.y + blockIdx.z * a.y_pair_pitch;
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
            xs[kk * kPitch + f] = (k_in && i0 + f < a.n) ? x[(long long)(i0 + f) * a.x_frame_pitch + k0 + kk] : 0.f;
            ys[kk * kPitch + f] = (k_in && j0 + f < a.m) ? y[(long long)(j0 + f) * a.y_frame_pitch + k0 + kk] : 0.f;
        }
        __syncthreads();
        for (int k = 0; k < kc; ++k) {
            const float4 xq = *reinterpret_cast<const float4*>(&xs[k * kPitch + 4 * ti]);
            const float4 yq = *reinterpret_cast<const float4*>(&ys[k * kPitch + 4 * tj]);
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
    float* out = a.cost + blockIdx.z * a.cost_pair_pitch;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + 4 * ti + r;
        float c4[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (METRIC == JSGX_METRIC_SQEUCLIDEAN) {
                c4[c] = acc[r][c];
            } else if (METRIC == JSGX_METRIC_EUCLIDEAN) {
                c4[c] = sqrtf(acc[r][c]);
            } else {
                const float den = sqrtf(nx[r]) * sqrtf(ny[c]);
                c4[c] = den == 0.f ? 1.0f : 1.0f - acc[r][c] / den;
            }
        }
        if (i >= a.n) continue;
        const int j = j0 + 4 * tj;
        float* row = out + (long long)i * a.cost_pitch;
        if (a.vec && j + 3 < a.m) {
            *reinterpret_cast<float4*>(row + j) = make_float4(c4[0], c4[1], c4[2], c4[3]);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (j + c < a.m) row[j + c] = c4[c];
        }
    }
}

}  // namespace jsgx

using namespace jsgx;

extern "C" int jsgx_cdist_launch(const jsgx_cdist_args* g, void* stream) {
    static const char* who = "jsgx_cdist_launch";
    int rc = cdist_check(g, who);
    if (rc != JSGX_OK) return rc;
    int dev = -1;
    if ((rc = current_device(&dev, who)) != JSGX_OK) return rc;
    // every refusal is behind us
    CdistArgs k{};
    k.x = g->x;
    k.x_frame_pitch = g->x_frame_pitch;
    k.x_pair_pitch = g->x_pair_pitch;
    k.y = g->y;
    k.y_frame_pitch = g->y_frame_pitch;
    k.y_pair_pitch = g->y_pair_pitch;
    k.cost = g->cost;
    k.cost_pitch = g->cost_pitch;
    k.cost_pair_pitch = g->pairs > 1 ? g->cost_pair_pitch : 0;
    k.n = g->n;
    k.m = g->m;
    k.K = g->n_features;
    // 16-byte stores where every row of every plane starts on a 16-byte boundary
    k.vec = ((reinterpret_cast<uintptr_t>(g->cost) | (uintptr_t)(4 * k.cost_pitch) | (uintptr_t)(4 * k.cost_pair_pitch)) & 15) == 0;
    const dim3 grid((unsigned)((g->m + kTile - 1) / kTile), (unsigned)((g->n + kTile - 1) / kTile), (unsigned)g->pairs);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (g->metric == JSGX_METRIC_SQEUCLIDEAN)
        hipLaunchKernelGGL(cdist_kernel<JSGX_METRIC_SQEUCLIDEAN>, grid, dim3(JSGX_CDIST_THREADS), 0, s, k);
    else if (g->metric == JSGX_METRIC_EUCLIDEAN)
        hipLaunchKernelGGL(cdist_kernel<JSGX_METRIC_EUCLIDEAN>, grid, dim3(JSGX_CDIST_THREADS), 0, s, k);
    else
        hipLaunchKernelGGL(cdist_kernel<JSGX_METRIC_COSINE>, grid, dim3(JSGX_CDIST_THREADS), 0, s, k);
    return finish_launch(who, hipGetLastError());
}
