// Shapley maps of a trained model (models_gcn.base_model.shapley / shapley_maps): sampled Shapley values of vertex groups.
// As for the occlusion maps, these are the memory-side kernels around the forward passes, which are the library's existing
// inference layers.
//
// A run has P permutations of the G groups, the same for every window, given as their inverse: rank[p][g] = the position of
// group g in permutation p.  Its rows are (window, permutation, prefix length) triples in that order, P (G + 1) per window:
// row r is window w = r / (P (G + 1)), permutation p = (r / (G + 1)) % P, prefix length j = r % (G + 1), and reveals the
// first j groups of permutation p: j = 0 is the baseline window, j = G the window itself.  r is also the row's index in the
// score table [S][P][G + 1].
//
//   rows:    staged windows [S][N][F] (caller's vertex order) -> plane storage [R][F][Mp] of rows r0 .. r0 + R in the internal
//            order: x[w_r][perm[i]][f] where gid[i] < 0 or rank[p_r][gid[i]] < j_r, else baseline[perm[i]][f]; the pad and
//            the rows past S P (G + 1) are 0.  A block writes SHAP_RC consecutive rows of one vertex tile: the window's tile
//            is gathered once per window the block touches and selected from for every prefix row of it
//   score:   logits [R][C] of those rows -> table[r] = s = z_c or log softmax(z)_c of the window's class c = cls[w]
//   reduce:  phi[w][g] = (1/P) sum_p (table[w][p][rank[p][g] + 1] - table[w][p][rank[p][g]]): float64 differences added in the
//            order of p, one float64 division, one rounding to float32
//
// The class of a window is known before its first row is scored: the driver runs one plain forward over the windows first
// under 'predicted'.  No atomics, fixed-order sums: reruns are bit-identical.  The row kernel is bounded by its stores.
#include <algorithm>

#include "saliency_tile.h"

namespace chebgcn {

constexpr int SHAP_RC = 16;    // rows a row-kernel workgroup writes from one vertex tile

// block (vertex tile, chunk of SHAP_RC rows of the pass)
__global__ void __launch_bounds__(SAL_T)
shapley_rows_kernel(const float* __restrict__ x, const int32_t* __restrict__ perm, const int32_t* __restrict__ gid,
                    const int32_t* __restrict__ rank, const float* __restrict__ x0, float* __restrict__ out, long long r0, int R,
                    int S, int P, int G, int N, int M, int Mp, int F) {
    extern __shared__ float tile[];             // x: [F][65], then (with a baseline) x0: [F][65]
    __shared__ int nodes[SAL_V];
    __shared__ int pos[SAL_V];                  // rank[p][group] of the tile's positions, -1: outside the game
    float* tile0 = tile + F * (SAL_V + 1);
    const long long G1 = (long long)G + 1;
    const int i0 = blockIdx.x * SAL_V;
    const int rb = blockIdx.y * SHAP_RC, re = min(R, rb + SHAP_RC);    // rows of this block, relative to r0
    load_nodes(nodes, perm, i0, M, N);
    int group = -1;                             // of position i0 + threadIdx.x, in the threads that fill pos
    if (threadIdx.x < SAL_V && i0 + threadIdx.x < M) {
        group = gid[i0 + threadIdx.x];
        if (group >= G) group = -1;
    }
    __syncthreads();
    if (x0) gather_tile(x0, 0, nodes, tile0, N, F);
    const int units = F * (SAL_V / 4);          // float4 stores per row of the tile
    long long wtile = -1;                       // the window whose tile LDS holds
    // t: the (window, permutation) pairs the block's rows lie in, t = w P + p
    for (long long t = (r0 + rb) / G1; t <= (r0 + re - 1) / G1; ++t) {
        const long long w = t / P;
        const int p = (int)(t - w * P);
        const bool live = w < S;
        __syncthreads();                        // nodes and x0 written / the previous pair's tile and pos read
        if (live && w != wtile) {
            gather_tile(x, (size_t)w * N * F, nodes, tile, N, F);
            wtile = w;
        }
        if (live && threadIdx.x < SAL_V) pos[threadIdx.x] = group >= 0 ? rank[(size_t)p * G + group] : -1;
        __syncthreads();
        const int ra = (int)std::max<long long>(rb, t * G1 - r0);
        const int rz = (int)std::min<long long>(re, (t + 1) * G1 - r0);
        for (int e = threadIdx.x; e < (rz - ra) * units; e += SAL_T) {
            const int rr = e / units, u = e - rr * units;
            const int f = u >> 4, q = (u & 15) * 4;
            const int i = i0 + q;
            if (i >= Mp) continue;              // Mp is a multiple of 32: a float4 is all in or all out
            const int r = ra + rr;
            const int j = (int)(r0 + r - t * G1);
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = f * (SAL_V + 1) + q + k;
                v[k] = !live ? 0.f : pos[q + k] < j ? tile[c] : x0 ? tile0[c] : 0.f;
            }
            *reinterpret_cast<float4*>(out + ((size_t)r * F + f) * Mp + i) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

// z_c or log softmax(z)_c: the arithmetic of occlusion.hip's scores (the maximum, then the sum of exp(z - max) in class order)
__device__ __forceinline__ float shapley_class_score(const float* __restrict__ z, int c, int C, int logprob) {
    if (!logprob) return z[c];
    float m = z[0];
    for (int k = 1; k < C; ++k) m = fmaxf(m, z[k]);
    float s = 0.f;
    for (int k = 0; k < C; ++k) s += expf(z[k] - m);
    return (z[c] - m) - logf(s);
}

// one thread per row of the pass
__global__ void __launch_bounds__(64)
shapley_score_kernel(const float* __restrict__ z, long long r0, int R, long long total, long long per, int C,
                     const long long* __restrict__ cls, int logprob, float* __restrict__ table) {
    const int rl = blockIdx.x * 64 + threadIdx.x;
    const long long r = r0 + rl;
    if (rl >= R || r >= total) return;
    const long long c = cls[r / per];
    table[r] = c < 0 || c >= C ? __builtin_nanf("") : shapley_class_score(z + (size_t)rl * C, (int)c, C, logprob);
}

// one thread per (window, group)
__global__ void __launch_bounds__(256)
shapley_reduce_kernel(const float* __restrict__ table, const int32_t* __restrict__ rank, long long SG, int P, int G,
                      float* __restrict__ phi) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= SG) return;
    const long long w = e / G;
    const int g = (int)(e - w * G);
    const long long G1 = (long long)G + 1;
    const float* s = table + (size_t)w * P * G1;
    double sum = 0.0;
    for (int p = 0; p < P; ++p) {
        const int k = rank[(size_t)p * G + g];
        if (k < 0 || k >= G) {                  // not a permutation: say so in the value, read nothing outside the table
            sum = __builtin_nan("");
            break;
        }
        sum += (double)s[p * G1 + k + 1] - (double)s[p * G1 + k];
    }
    phi[e] = (float)(sum / (double)P);
}

}  // namespace chebgcn

using namespace chebgcn;

// the LDS of the row kernel: the x and x0 tiles ([F][65] floats each) and the two [64] int tables
extern "C" int chebgcn_shapley_supported(int F) {
    return F > 0 && 2 * (size_t)F * (SAL_V + 1) * sizeof(float) + 2 * SAL_V * sizeof(int) <= 64 * 1024 ? 1 : 0;
}

extern "C" int chebgcn_shapley_rows(const float* x, const int32_t* perm, const int32_t* gid, const int32_t* rank,
                                    const float* baseline, float* out, int64_t r0, int R, int S, int P, int G, int N, int M, int F,
                                    chebgcn_stream stream_) {
    CG_REQUIRE(x && gid && rank && out, "shapley_rows: NULL argument");
    CG_REQUIRE(r0 >= 0 && R > 0 && R <= 65535 && S > 0 && P > 0 && G > 0 && N > 0 && M > 0 && F > 0, "shapley_rows: bad shape");
    CG_REQUIRE((long long)P * ((long long)G + 1) < (1ll << 31), "shapley_rows: P (G + 1) = %lld rows per window, limit 2^31 - 1",
               (long long)P * ((long long)G + 1));
    CG_REQUIRE(perm || M == N, "shapley_rows: identity permutation needs M == N");
    CG_REQUIRE(chebgcn_shapley_supported(F), "shapley_rows: F=%d too large (chebgcn_shapley_supported)", F);
    CG_REQUIRE(((uintptr_t)out & 15) == 0, "shapley_rows: out must be 16-byte aligned");
    const size_t lds = (baseline ? 2 : 1) * (size_t)F * (SAL_V + 1) * sizeof(float);
    const int Mp = plane_stride(M);
    dim3 grid((Mp + SAL_V - 1) / SAL_V, (R + SHAP_RC - 1) / SHAP_RC);
    note_dispatch("shapley_rows_kernel");
    hipLaunchKernelGGL(shapley_rows_kernel, grid, dim3(SAL_T), lds, (hipStream_t)stream_, x, perm, gid, rank, baseline, out,
                       (long long)r0, R, S, P, G, N, M, Mp, F);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_shapley_score(const float* logits, int64_t r0, int R, int S, int P, int G, int C, const int64_t* cls,
                                     int score, float* table, chebgcn_stream stream_) {
    CG_REQUIRE(logits && cls && table, "shapley_score: NULL argument");
    CG_REQUIRE(r0 >= 0 && R > 0 && S > 0 && P > 0 && G > 0 && C > 0, "shapley_score: bad shape");
    CG_REQUIRE(score == CHEBGCN_SCORE_LOGIT || score == CHEBGCN_SCORE_LOGPROB, "shapley_score: score %d", score);
    const long long per = (long long)P * ((long long)G + 1);
    CG_REQUIRE(per < (1ll << 31), "shapley_score: P (G + 1) = %lld rows per window, limit 2^31 - 1", per);
    note_dispatch(score == CHEBGCN_SCORE_LOGPROB ? "shapley_score_kernel<logprob>" : "shapley_score_kernel<logit>");
    hipLaunchKernelGGL(shapley_score_kernel, dim3((R + 63) / 64), dim3(64), 0, (hipStream_t)stream_, logits, (long long)r0, R,
                       (long long)S * per, per, C, (const long long*)cls, score == CHEBGCN_SCORE_LOGPROB ? 1 : 0, table);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_shapley_reduce(const float* table, const int32_t* rank, int S, int P, int G, float* phi,
                                      chebgcn_stream stream_) {
    CG_REQUIRE(table && rank && phi, "shapley_reduce: NULL argument");
    CG_REQUIRE(S > 0 && P > 0 && G > 0, "shapley_reduce: bad shape");
    const long long SG = (long long)S * G;
    CG_REQUIRE((SG + 255) / 256 < (1ll << 31), "shapley_reduce: S G = %lld is more than one launch covers", SG);
    note_dispatch("shapley_reduce_kernel");
    hipLaunchKernelGGL(shapley_reduce_kernel, dim3((unsigned)((SG + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, table, rank,
                       SG, P, G, phi);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}
