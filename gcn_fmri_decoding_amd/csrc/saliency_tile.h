// What saliency.hip and occlusion.hip share: the row -> plane tile gather through LDS (64 internal positions, [F][65] floats)
// and the fixed-order float64 per-class sums over per-window rows.
#pragma once
#include "common.h"

namespace chebgcn {

constexpr int SAL_T = 256;     // threads of the tile workgroups
constexpr int SAL_V = 64;      // vertices per tile

// gathers the [F][64] tile of window row `src` (vertex nodes[q], N = none -> 0) into LDS, four loads in flight per thread
__device__ __forceinline__ void gather_tile(const float* __restrict__ x, size_t src, const int* nodes, float* tile, int N, int F) {
    for (int e0 = threadIdx.x; e0 < SAL_V * F; e0 += 4 * SAL_T) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + SAL_T * u, ec = e < SAL_V * F ? e : 0;
            const int q = ec / F, f = ec - q * F;
            const int node = nodes[q];
            const float t = x[src + (size_t)(node < N ? node : 0) * F + f];
            v[u] = node < N ? t : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + SAL_T * u;
            if (e < SAL_V * F) {
                const int q = e / F, f = e - q * F;
                tile[f * (SAL_V + 1) + q] = v[u];
            }
        }
    }
}

__device__ __forceinline__ void load_nodes(int* nodes, const int32_t* __restrict__ perm, int i0, int M, int N) {
    if (threadIdx.x < SAL_V) {
        const int i = i0 + threadIdx.x;
        const int node = i < M ? (perm ? perm[i] : i) : N;
        nodes[threadIdx.x] = node >= 0 && node < N ? node : N;
    }
}

// acc[k][e] += the sum, windows in order, of rows[w][e] over the windows with cls[w] == k (saliency_class_sum_kernel;
// rows [nw][NF] float32, cls int64 [nw], acc float64 [ncls][NF]).  Enqueues one launch on `stream`; no error check.
void launch_class_sum(const float* rows, const int64_t* cls, double* acc, int nw, long long NF, int ncls, hipStream_t stream);

}  // namespace chebgcn
