// Grad-CAM maps of a trained model (models_gcn.base_model.gradcam / gradcam_maps): the two kernels behind the pass that stops
// the input gradient at a conv layer's output.
//
// A is the layer's activation and G = ds/dA its gradient, both plane storage [B][F][Mp] over the N vertices of the layer's
// level, in that level's internal order; the pad [N, Mp) of a plane is scratch (it may hold NaN) and is never summed.
//
//   weights: alpha[r][f] = (1/N) sum_{i<N} G[r][f][i]   (float64 partial sums in a fixed order, rounded once)
//   map:     cam_i = sum_f alpha[r][f] A[r][f][i]  ('gradcam')  or  sum_f G[r][f][i] A[r][f][i]  ('grad_x_activation'),
//            filters in order, max(0, .) with relu; level vertex i is reference vertex j = order[i] (identity without a
//            table), which covers the P input vertices [j P, (j + 1) P): out[r][j P + q] = cam_i, q < P.
//
// No atomics, fixed-order sums: reruns are bit-identical.  Both kernels stream their operands once with 16-byte loads along
// the plane; the map kernel stages a tile's values in LDS so that its stores run along the output row.
#include "common.h"

namespace chebgcn {

constexpr int CAM_T = 256;              // threads of both kernels
constexpr int CAM_V = 4 * CAM_T;        // level vertices of a map tile: four consecutive ones per thread (one float4)

// block (r, f): one plane of G
__global__ void __launch_bounds__(CAM_T)
gradcam_weights_kernel(const float* __restrict__ G, int F, int N, int Mp, float* __restrict__ alpha) {
    __shared__ double part[CAM_T / 64];
    const int plane = blockIdx.x;                       // r * F + f
    const float* g = G + (size_t)plane * Mp;
    double s = 0.0;
    for (int i = 4 * threadIdx.x; i < N; i += 4 * CAM_T) {
        const float4 v = *reinterpret_cast<const float4*>(g + i);      // Mp is a multiple of 32: in bounds, 16-byte aligned
        s += (double)v.x;
        if (i + 1 < N) s += (double)v.y;
        if (i + 2 < N) s += (double)v.z;
        if (i + 3 < N) s += (double)v.w;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < CAM_T / 64; ++w) t += part[w];
        alpha[plane] = (float)(t / (double)N);
    }
}

// block (tile of CAM_V level vertices, window r)
template <bool PerVertex>
__global__ void __launch_bounds__(CAM_T)
gradcam_map_kernel(const float* __restrict__ A, const float* __restrict__ G, const float* __restrict__ alpha,
                   const int32_t* __restrict__ order, int F, int N, int Mp, int logP, int relu, float* __restrict__ out,
                   long long ldo) {
    __shared__ float cam[CAM_V];
    __shared__ int ref[CAM_V];
    const int r = blockIdx.y;
    const int i0 = blockIdx.x * CAM_V;
    const int i = i0 + 4 * threadIdx.x;
    float c[4] = {0.f, 0.f, 0.f, 0.f};
    if (i < Mp) {
        const size_t base = (size_t)r * F * Mp + i;
#pragma unroll 4
        for (int f = 0; f < F; ++f) {
            const float4 a = *reinterpret_cast<const float4*>(A + base + (size_t)f * Mp);
            float4 w;
            if (PerVertex) {
                w = *reinterpret_cast<const float4*>(G + base + (size_t)f * Mp);
            } else {
                const float al = alpha[(size_t)r * F + f];
                w = make_float4(al, al, al, al);
            }
            c[0] = fmaf(w.x, a.x, c[0]);
            c[1] = fmaf(w.y, a.y, c[1]);
            c[2] = fmaf(w.z, a.z, c[2]);
            c[3] = fmaf(w.w, a.w, c[3]);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int v = i + k;
        int j = -1;
        if (v < N) {
            j = order ? order[v] : v;
            if (j < 0 || j >= N) j = -1;                // (a malformed table writes nothing)
        }
        cam[4 * threadIdx.x + k] = relu ? fmaxf(c[k], 0.f) : c[k];
        ref[4 * threadIdx.x + k] = j;
    }
    __syncthreads();
    // the tile's vertices times P consecutive outputs each: along the row where the order is the identity, runs of P otherwise
    const int nv = min(CAM_V, N - i0);
    const int total = nv << logP;
    const int P1 = (1 << logP) - 1;
    float* o = out + (size_t)r * ldo;
    for (int e = threadIdx.x; e < total; e += CAM_T) {
        const int q = e >> logP;
        const int j = ref[q];
        if (j >= 0) o[((size_t)j << logP) + (e & P1)] = cam[q];
    }
}

}  // namespace chebgcn

using namespace chebgcn;

extern "C" int chebgcn_gradcam_weights(const float* G, int nw, int F, int N, float* alpha, chebgcn_stream stream_) {
    CG_REQUIRE(G && alpha, "gradcam_weights: NULL argument");
    CG_REQUIRE(nw > 0 && F > 0 && N > 0 && (long long)nw * F <= 0x7fffffffLL, "gradcam_weights: bad shape");
    CG_REQUIRE(((uintptr_t)G & 15) == 0, "gradcam_weights: G must be 16-byte aligned");
    note_dispatch("gradcam_weights_kernel");
    hipLaunchKernelGGL(gradcam_weights_kernel, dim3(nw * F), dim3(CAM_T), 0, (hipStream_t)stream_, G, F, N, plane_stride(N),
                       alpha);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_gradcam_map(const float* A, const float* G, const float* alpha, const int32_t* order, int nw, int F, int N,
                                   int P, int relu, float* out, int64_t ldo, chebgcn_stream stream_) {
    CG_REQUIRE(A && out && (G != nullptr) != (alpha != nullptr), "gradcam_map: NULL argument (exactly one of G and alpha)");
    CG_REQUIRE(nw > 0 && nw <= 65535 && F > 0 && N > 0 && P > 0 && (P & (P - 1)) == 0, "gradcam_map: bad shape");
    CG_REQUIRE(ldo >= (int64_t)N * P, "gradcam_map: output rows of %lld floats hold fewer than N P = %lld", (long long)ldo,
               (long long)N * P);
    CG_REQUIRE(((uintptr_t)A & 15) == 0 && ((uintptr_t)G & 15) == 0, "gradcam_map: A and G must be 16-byte aligned");
    int logP = 0;
    while ((1 << logP) < P) ++logP;
    const int Mp = plane_stride(N);
    dim3 grid((N + CAM_V - 1) / CAM_V, nw);
    if (G) {
        note_dispatch("gradcam_map_kernel<grad_x_activation>");
        hipLaunchKernelGGL(gradcam_map_kernel<true>, grid, dim3(CAM_T), 0, (hipStream_t)stream_, A, G, alpha, order, F, N, Mp,
                           logP, relu ? 1 : 0, out, (long long)ldo);
    } else {
        note_dispatch("gradcam_map_kernel<gradcam>");
        hipLaunchKernelGGL(gradcam_map_kernel<false>, grid, dim3(CAM_T), 0, (hipStream_t)stream_, A, G, alpha, order, F, N, Mp,
                           logP, relu ? 1 : 0, out, (long long)ldo);
    }
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}
