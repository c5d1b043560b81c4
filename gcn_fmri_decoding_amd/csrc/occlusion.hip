// Occlusion maps of a trained model (models_gcn.base_model.occlusion / occlusion_maps): the memory-side kernels around the
// forward passes, which are the library's existing inference layers.
//
// The rows of an occlusion run are (window, group) pairs in window-major order, G + 1 rows per window: row r is window
// w = r / (G + 1), slot j = r % (G + 1); slot 0 is the window itself (group g = G, which matches no vertex), slot j >= 1
// occludes group g = j - 1.  The reference row thus precedes the rows it is compared with, in the same pass or an earlier one.
//
//   rows:    staged windows [S][N][F] (caller's vertex order) -> plane storage [R][F][Mp] of rows r0 .. r0 + R in the internal
//            order: baseline[perm[i]][f] where gid[i] == g_r, else x[w_r][perm[i]][f]; the pad and the rows past S (G + 1) are 0
//   score:   logits [R][C] of those rows -> drop[w][g] = s(reference row) - s(row), s = z_c or log softmax(z)_c of the
//            window's class c = cls[w]; a reference row writes its own score to ref[w] for the passes after it
//   class sums: drop [S][G] -> acc[k][g] += the sum, windows in order, over the windows of class k (saliency_class_sum_kernel)
//
// No atomics, fixed-order sums: reruns are bit-identical.  The row kernel is bounded by its stores.
#include <algorithm>

#include "saliency_tile.h"

namespace chebgcn {

constexpr int OCC_RC = 8;      // rows a row-kernel workgroup writes from one window tile

// block (vertex tile, chunk of OCC_RC rows of the pass)
__global__ void __launch_bounds__(SAL_T)
occlusion_rows_kernel(const float* __restrict__ x, const int32_t* __restrict__ perm, const int32_t* __restrict__ gid,
                      const float* __restrict__ x0, float* __restrict__ out, long long r0, int R, int S, int G, int N, int M,
                      int Mp, int F) {
    extern __shared__ float tile[];             // x: [F][65], then x0: [F][65]
    __shared__ int nodes[SAL_V];
    __shared__ int groups[SAL_V];
    float* tile0 = tile + F * (SAL_V + 1);
    const long long G1 = (long long)G + 1;
    const int i0 = blockIdx.x * SAL_V;
    const int rb = blockIdx.y * OCC_RC, re = min(R, rb + OCC_RC);      // rows of this block, relative to r0
    load_nodes(nodes, perm, i0, M, N);
    if (threadIdx.x < SAL_V) {
        const int i = i0 + threadIdx.x;
        groups[threadIdx.x] = i < M ? gid[i] : -1;
    }
    __syncthreads();
    if (x0) gather_tile(x0, 0, nodes, tile0, N, F);
    const int units = F * (SAL_V / 4);          // float4 stores per row of the tile
    for (long long w = (r0 + rb) / G1; w <= (r0 + re - 1) / G1; ++w) {
        const bool live = w < S;
        __syncthreads();                        // nodes, groups and x0 written / the previous window's tile read
        if (live) gather_tile(x, (size_t)w * N * F, nodes, tile, N, F);
        __syncthreads();
        const int ra = (int)std::max<long long>(rb, w * G1 - r0);
        const int rz = (int)std::min<long long>(re, (w + 1) * G1 - r0);
        for (int e = threadIdx.x; e < (rz - ra) * units; e += SAL_T) {
            const int rr = e / units, u = e - rr * units;
            const int f = u >> 4, q = (u & 15) * 4;
            const int i = i0 + q;
            if (i >= Mp) continue;              // Mp is a multiple of 32: a float4 is all in or all out
            const int r = ra + rr;
            const long long j = r0 + r - w * G1;
            const int g = j == 0 ? G : (int)(j - 1);
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int t = f * (SAL_V + 1) + q + k;
                v[k] = !live ? 0.f : groups[q + k] != g ? tile[t] : x0 ? tile0[t] : 0.f;
            }
            *reinterpret_cast<float4*>(out + ((size_t)r * F + f) * Mp + i) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

// z_c or log softmax(z)_c (the maximum, then the sum of exp(z - max) in class order)
__device__ __forceinline__ float class_score(const float* __restrict__ z, int c, int C, int logprob) {
    if (!logprob) return z[c];
    float m = z[0];
    for (int k = 1; k < C; ++k) m = fmaxf(m, z[k]);
    float s = 0.f;
    for (int k = 0; k < C; ++k) s += expf(z[k] - m);
    return (z[c] - m) - logf(s);
}

// one thread per row of the pass
__global__ void __launch_bounds__(64)
occlusion_score_kernel(const float* __restrict__ z, long long r0, int R, int S, int G, int C, const long long* __restrict__ cls,
                       int logprob, float* __restrict__ ref, float* __restrict__ drop) {
    const int rl = blockIdx.x * 64 + threadIdx.x;
    const long long G1 = (long long)G + 1;
    const long long r = r0 + rl;
    if (rl >= R || r >= (long long)S * G1) return;
    const long long w = r / G1, j = r - w * G1;
    const long long c = cls[w];
    const bool bad = c < 0 || c >= C;
    const float s = bad ? __builtin_nanf("") : class_score(z + (size_t)rl * C, (int)c, C, logprob);
    if (j == 0) {
        ref[w] = s;
        return;
    }
    // the reference row: in this pass (scored here again, the same arithmetic), or written by an earlier pass's launch
    const long long rref = w * G1 - r0;
    const float sref = rref >= 0 ? (bad ? __builtin_nanf("") : class_score(z + (size_t)rref * C, (int)c, C, logprob)) : ref[w];
    drop[(size_t)w * G + (j - 1)] = sref - s;
}

}  // namespace chebgcn

using namespace chebgcn;

// the LDS of the row kernel: the x and x0 tiles ([F][65] floats each) and the two [64] int tables
extern "C" int chebgcn_occlusion_supported(int F) {
    return F > 0 && 2 * (size_t)F * (SAL_V + 1) * sizeof(float) + 2 * SAL_V * sizeof(int) <= 64 * 1024 ? 1 : 0;
}

extern "C" int chebgcn_occlusion_rows(const float* x, const int32_t* perm, const int32_t* gid, const float* baseline, float* out,
                                      int64_t r0, int R, int S, int G, int N, int M, int F, chebgcn_stream stream_) {
    CG_REQUIRE(x && gid && out, "occlusion_rows: NULL argument");
    CG_REQUIRE(r0 >= 0 && R > 0 && R <= 65535 && S > 0 && G > 0 && N > 0 && M > 0 && F > 0, "occlusion_rows: bad shape");
    CG_REQUIRE(perm || M == N, "occlusion_rows: identity permutation needs M == N");
    CG_REQUIRE(chebgcn_occlusion_supported(F), "occlusion_rows: F=%d too large (chebgcn_occlusion_supported)", F);
    CG_REQUIRE(((uintptr_t)out & 15) == 0, "occlusion_rows: out must be 16-byte aligned");
    const size_t lds = 2 * (size_t)F * (SAL_V + 1) * sizeof(float);
    const int Mp = plane_stride(M);
    dim3 grid((Mp + SAL_V - 1) / SAL_V, (R + OCC_RC - 1) / OCC_RC);
    note_dispatch("occlusion_rows_kernel");
    hipLaunchKernelGGL(occlusion_rows_kernel, grid, dim3(SAL_T), lds, (hipStream_t)stream_, x, perm, gid, baseline, out,
                       (long long)r0, R, S, G, N, M, Mp, F);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_occlusion_score(const float* logits, int64_t r0, int R, int S, int G, int C, const int64_t* cls, int score,
                                       float* ref, float* drop, chebgcn_stream stream_) {
    CG_REQUIRE(logits && cls && ref && drop, "occlusion_score: NULL argument");
    CG_REQUIRE(r0 >= 0 && R > 0 && S > 0 && G > 0 && C > 0, "occlusion_score: bad shape");
    CG_REQUIRE(score == CHEBGCN_SCORE_LOGIT || score == CHEBGCN_SCORE_LOGPROB, "occlusion_score: score %d", score);
    note_dispatch(score == CHEBGCN_SCORE_LOGPROB ? "occlusion_score_kernel<logprob>" : "occlusion_score_kernel<logit>");
    hipLaunchKernelGGL(occlusion_score_kernel, dim3((R + 63) / 64), dim3(64), 0, (hipStream_t)stream_, logits, (long long)r0, R,
                       S, G, C, (const long long*)cls, score == CHEBGCN_SCORE_LOGPROB ? 1 : 0, ref, drop);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_occlusion_class_sums(const float* drop, const int64_t* cls, int S, int G, int ncls, double* acc,
                                            chebgcn_stream stream_) {
    CG_REQUIRE(drop && cls && acc, "occlusion_class_sums: NULL argument");
    CG_REQUIRE(S > 0 && G > 0 && ncls > 0 && ncls <= 65535, "occlusion_class_sums: bad shape");
    note_dispatch("saliency_class_sum_kernel");
    launch_class_sum(drop, cls, acc, S, G, ncls, (hipStream_t)stream_);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}
