// libjsgx.so, the pairwise cost of two feature sequences (include/jsgx.h section 2): the kernel and its launcher.  The refusals and the
// plan are in jsgx_dtw_host.cpp.
//
// The costs of a workgroup's 64 x 64 tile are jsgx_cost_tile.h's; "cdist_64x64" stores them.  Frames past N or M are never stored.  A row
// of the tile goes out as 16 lanes x 16 bytes = one 256-byte line (as 16-byte stores where cost is so aligned).
#include <hip/hip_runtime.h>

#include "jsgx_cost_tile.h"

namespace jsgx {

struct CdistArgs {
    Plane<const float> x, y;
    Plane<float> cost;
    int n, m, K, vec;
};

template <int METRIC>
__global__ __launch_bounds__(JSGX_CDIST_THREADS) void cdist_kernel(CdistArgs a) {
    __shared__ __attribute__((aligned(16))) float xs[kPanel * kPitch];
    __shared__ __attribute__((aligned(16))) float ys[kPanel * kPitch];
    const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
    const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
    const CostTile t = cost_tile<METRIC>({a.x.row(blockIdx.z, 0), a.x.pitch, a.y.row(blockIdx.z, 0), a.y.pitch, a.n, a.m, a.K, xs, ys}, i0, j0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + 4 * ti + r, j = j0 + 4 * tj;
        if (i >= a.n) continue;
        float* row = a.cost.row(blockIdx.z, i);
        if (a.vec && j + 3 < a.m) {
            *reinterpret_cast<float4*>(row + j) = make_float4(t.c[r][0], t.c[r][1], t.c[r][2], t.c[r][3]);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (j + c < a.m) row[j + c] = t.c[r][c];
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
    CdistArgs k{sequence_of(g->x, g->x_frame_pitch, g->x_pair_pitch), sequence_of(g->y, g->y_frame_pitch, g->y_pair_pitch),
                plane_of(g->cost, g->cost_pitch, g->cost_pair_pitch, g->pairs), g->n, g->m, g->n_features, 0};
    // 16-byte stores where every row of every plane starts on a 16-byte boundary
    k.vec = ((reinterpret_cast<uintptr_t>(g->cost) | (uintptr_t)(4 * k.cost.pitch) | (uintptr_t)(4 * k.cost.pair_pitch)) & 15) == 0;
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
