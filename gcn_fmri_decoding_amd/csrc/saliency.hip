// Saliency maps of a trained cgcnn (models_gcn.base_model.saliency / saliency_maps): the three memory-side kernels around the
// input-gradient pass.  The pass itself -- forward with the ReLU masks, then the training step's dx kernels only -- is the
// library's existing layers.
//
//   seed:    logits [B][C] + target (given, or the first maximum) -> d score / d logits [B][C] and the chosen class
//            score 'logit': e_t;  'logprob' (log softmax(z)_t): e_t - softmax(z)
//   path:    staged windows [S][N][F] (caller's vertex order) -> plane storage [R][F][Mp] in the model's internal order, row
//            w*steps + j = x0 + a_j (x - x0), a_j = (j + 1/2) / steps (the midpoint rule of integrated gradients); the rows
//            behind the windows and the pad of every plane are written as 0
//   reduce:  input-gradient planes [nw*steps][F][Mp] (internal order) -> per-window rows [nw][N][F] in the caller's order
//            (the steps of a window summed in order, times 1, x or (x - x0) / steps, optionally |.|), and optionally the
//            per-class sums of those rows into a float64 accumulator [ncls][N][F], windows in order
//
// Every sum runs in a fixed order (no atomics): repeated calls are bit-identical.  All three are HBM-side passes; the
// plane <-> row change goes through an LDS tile of 64 vertices, as chebgcn_perm_data does.
#include <algorithm>

#include "saliency_tile.h"

namespace chebgcn {

// one thread per row of logits; C is small (the classes of the head)
__global__ void __launch_bounds__(64)
saliency_seed_kernel(const float* __restrict__ z, const long long* __restrict__ targets, int rep, int nvalid, int logprob,
                     float* __restrict__ dz, long long* __restrict__ cls, int B, int C) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= B) return;
    const float* row = z + (size_t)r * C;
    float* drow = dz ? dz + (size_t)r * C : nullptr;
    if (r >= nvalid) {                          // padding rows: no gradient, no class
        if (drow)
            for (int c = 0; c < C; ++c) drow[c] = 0.f;
        return;
    }
    long long t;
    if (targets) {
        t = targets[r / rep];
    } else {
        // torch.argmax's rule (what prediction() returns): the first maximum, a NaN counting as the largest value
        float best = row[0];
        t = 0;
        for (int c = 1; c < C; ++c) {
            const float v = row[c];
            if (best == best && (v > best || v != v)) {
                best = v;
                t = c;
            }
        }
    }
    const bool bad = t < 0 || t >= C;           // the caller's error: a NaN row, nothing read or written past the row
    if (cls && r % rep == 0) cls[r / rep] = t;
    if (!drow) return;
    if (bad) {
        for (int c = 0; c < C; ++c) drow[c] = __builtin_nanf("");
        return;
    }
    if (!logprob) {
        for (int c = 0; c < C; ++c) drow[c] = c == t ? 1.f : 0.f;
        return;
    }
    // 1 - p_t as the sum of the other classes' shares (as softmax_xent_kernel does): a confident row (p_t -> 1) keeps its
    // relative precision instead of cancelling in fp32
    float m = row[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, row[c]);
    float s = 0.f, so = 0.f;
    for (int c = 0; c < C; ++c) {
        const float e = expf(row[c] - m);
        s += e;
        so += c == t ? 0.f : e;
    }
    const float inv = 1.f / s;
    for (int c = 0; c < C; ++c) drow[c] = c == t ? so * inv : -expf(row[c] - m) * inv;
}

// block (vertex tile, window w): rows w*steps .. w*steps + steps - 1 of the output
__global__ void __launch_bounds__(SAL_T)
saliency_path_kernel(const float* __restrict__ x, const int32_t* __restrict__ perm, const int32_t* __restrict__ sample,
                     const float* __restrict__ x0, float* __restrict__ out, int N, int M, int Mp, int F, int nw, int steps,
                     int R) {
    extern __shared__ float tile[];             // x: [F][65], then x0: [F][65]
    __shared__ int nodes[SAL_V];
    float* tile0 = tile + F * (SAL_V + 1);
    const int w = blockIdx.y;
    const int i0 = blockIdx.x * SAL_V;
    const bool live = w < nw;
    load_nodes(nodes, perm, i0, M, N);
    __syncthreads();
    if (live) {
        gather_tile(x, (size_t)sample[w] * N * F, nodes, tile, N, F);
        if (x0) gather_tile(x0, 0, nodes, tile0, N, F);
    }
    __syncthreads();
    const float inv = 1.f / (float)steps;
    for (int j = 0; j < steps; ++j) {
        const long long r = (long long)w * steps + j;
        if (r >= R) break;
        const float a = ((float)j + 0.5f) * inv;
        float* orow = out + (size_t)r * F * Mp;
        for (int e = threadIdx.x; e < SAL_V * F; e += SAL_T) {
            const int f = e >> 6, q = e & 63;
            const int i = i0 + q;
            if (i < Mp) {
                float v = 0.f;
                if (live) {
                    const float b = x0 ? tile0[f * (SAL_V + 1) + q] : 0.f;
                    v = b + a * (tile[f * (SAL_V + 1) + q] - b);
                }
                orow[(size_t)f * Mp + i] = v;
            }
        }
    }
}

// block (vertex tile, windows blockIdx.y, + gridDim.y, ...)
__global__ void __launch_bounds__(SAL_T)
saliency_rows_kernel(const float* __restrict__ dx, const float* __restrict__ x, const int32_t* __restrict__ perm,
                     const int32_t* __restrict__ sample, const float* __restrict__ x0, float* __restrict__ out, int N, int M,
                     int Mp, int F, int nw, int steps, int method, int absval) {
    extern __shared__ float tile[];             // [F][65]: the step sums of the window's tile
    __shared__ int nodes[SAL_V];
    const int i0 = blockIdx.x * SAL_V;
    load_nodes(nodes, perm, i0, M, N);
    const float inv = 1.f / (float)steps;
    for (int w = blockIdx.y; w < nw; w += gridDim.y) {
        __syncthreads();                        // nodes written / the previous window's tile read
        for (int e = threadIdx.x; e < SAL_V * F; e += SAL_T) {
            const int f = e >> 6, q = e & 63;
            const int i = i0 + q;
            float s = 0.f;
            if (i < M) {
                const float* p = dx + ((size_t)w * steps * F + f) * Mp + i;
#pragma unroll 4
                for (int j = 0; j < steps; ++j) s += p[(size_t)j * F * Mp];
            }
            tile[f * (SAL_V + 1) + q] = s;
        }
        __syncthreads();
        const size_t src = method ? (size_t)sample[w] * N * F : 0;
        float* orow = out + (size_t)w * N * F;
        for (int e = threadIdx.x; e < SAL_V * F; e += SAL_T) {
            const int q = e / F, f = e - q * F;
            const int node = nodes[q];
            if (node < N) {
                const size_t o = (size_t)node * F + f;
                const float g = tile[f * (SAL_V + 1) + q];
                float v = g;
                if (method == 1) {
                    v = x[src + o] * g;
                } else if (method == 2) {
                    const float d = x[src + o] - (x0 ? x0[o] : 0.f);
                    v = d * (g * inv);
                }
                orow[o] = absval ? fabsf(v) : v;
            }
        }
    }
}

// block (256 elements of a row, class k): acc[k][e] += sum over the windows of class k, in window order, of rows[w][e]
__global__ void __launch_bounds__(SAL_T)
saliency_class_sum_kernel(const float* __restrict__ rows, const long long* __restrict__ cls, double* __restrict__ acc, int nw,
                          long long NF) {
    __shared__ long long cs[1024];
    const long long k = blockIdx.y;
    const long long e = (long long)blockIdx.x * SAL_T + threadIdx.x;
    const bool in = e < NF;
    double s = 0.0;
    bool any = false;
    for (int w0 = 0; w0 < nw; w0 += 1024) {
        __syncthreads();
        for (int t = threadIdx.x; t < 1024 && w0 + t < nw; t += SAL_T) cs[t] = cls[w0 + t];
        __syncthreads();
        const int n = min(1024, nw - w0);
        for (int t = 0; t < n; ++t) {
            if (cs[t] == k) {                   // the same in every lane
                any = true;
                if (in) s += (double)rows[(size_t)(w0 + t) * NF + e];
            }
        }
    }
    if (any && in) acc[k * NF + e] += s;
}

void launch_class_sum(const float* rows, const int64_t* cls, double* acc, int nw, long long NF, int ncls, hipStream_t stream) {
    hipLaunchKernelGGL(saliency_class_sum_kernel, dim3((unsigned)((NF + SAL_T - 1) / SAL_T), ncls), dim3(SAL_T), 0, stream, rows,
                       (const long long*)cls, acc, nw, NF);
}

}  // namespace chebgcn

using namespace chebgcn;

// the LDS tiles: the path kernel holds x and x0 ([F][65] floats each), the reduce kernel one
extern "C" int chebgcn_saliency_supported(int F) {
    return F > 0 && 2 * (size_t)F * (SAL_V + 1) * sizeof(float) <= 64 * 1024 ? 1 : 0;
}

extern "C" int chebgcn_saliency_seed(const float* logits, const int64_t* targets, int rep, int nvalid, int score,
                                     float* dlogits, int64_t* cls_out, int B, int C, chebgcn_stream stream_) {
    CG_REQUIRE(logits && (dlogits || cls_out), "saliency_seed: NULL argument");
    CG_REQUIRE(B > 0 && C > 0 && rep > 0 && nvalid >= 0 && nvalid <= B, "saliency_seed: bad shape");
    CG_REQUIRE(score == CHEBGCN_SCORE_LOGIT || score == CHEBGCN_SCORE_LOGPROB, "saliency_seed: score %d", score);
    note_dispatch(targets ? "saliency_seed_kernel<target>" : "saliency_seed_kernel<argmax>");
    hipLaunchKernelGGL(saliency_seed_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream_, logits,
                       (const long long*)targets, rep, nvalid, score == CHEBGCN_SCORE_LOGPROB ? 1 : 0, dlogits,
                       (long long*)cls_out, B, C);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_saliency_path(const float* x, const int32_t* perm, const int32_t* sample, const float* baseline,
                                     float* out, int nw, int steps, int R, int N, int M, int F, chebgcn_stream stream_) {
    CG_REQUIRE(x && sample && out, "saliency_path: NULL argument");
    CG_REQUIRE(nw > 0 && steps > 0 && N > 0 && M > 0 && F > 0 && R <= 65535 && (int64_t)nw * steps <= R,
               "saliency_path: bad shape");
    CG_REQUIRE(perm || M == N, "saliency_path: identity permutation needs M == N");
    CG_REQUIRE(chebgcn_saliency_supported(F), "saliency_path: F=%d too large (chebgcn_saliency_supported)", F);
    const size_t lds = 2 * (size_t)F * (SAL_V + 1) * sizeof(float);
    const int Mp = plane_stride(M);
    dim3 grid((Mp + SAL_V - 1) / SAL_V, (R + steps - 1) / steps);
    note_dispatch("saliency_path_kernel");
    hipLaunchKernelGGL(saliency_path_kernel, grid, dim3(SAL_T), lds, (hipStream_t)stream_, x, perm, sample, baseline, out, N, M,
                       Mp, F, nw, steps, R);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_saliency_reduce(const float* dx, const float* x, const int32_t* perm, const int32_t* sample,
                                       const float* baseline, int nw, int steps, int M, int F, int method, int absolute,
                                       float* out, const int64_t* cls, int ncls, double* acc, chebgcn_stream stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CG_REQUIRE(dx && out, "saliency_reduce: NULL argument");
    CG_REQUIRE(method == CHEBGCN_SAL_GRADIENT || method == CHEBGCN_SAL_GRAD_X_INPUT || method == CHEBGCN_SAL_INTEGRATED,
               "saliency_reduce: method %d", method);
    CG_REQUIRE(method == CHEBGCN_SAL_GRADIENT || (x && sample), "saliency_reduce: this method reads the windows (x, sample)");
    CG_REQUIRE(nw > 0 && nw <= 65535 && steps > 0 && M > 0 && F > 0 && (int64_t)nw * steps <= 65535,
               "saliency_reduce: bad shape");
    CG_REQUIRE(!acc || (cls && ncls > 0 && ncls <= 65535), "saliency_reduce: the class sums need cls and ncls");
    CG_REQUIRE(chebgcn_saliency_supported(F), "saliency_reduce: F=%d too large (chebgcn_saliency_supported)", F);
    const size_t lds = (size_t)F * (SAL_V + 1) * sizeof(float);
    const int Mp = plane_stride(M);
    const int tiles = (M + SAL_V - 1) / SAL_V;
    // enough workgroups for the machine: windows spread over the grid's second axis, each block walks its own
    const int wy = std::max(1, std::min(nw, (4 * 256 + tiles - 1) / tiles));
    note_dispatch("saliency_rows_kernel");
    hipLaunchKernelGGL(saliency_rows_kernel, dim3(tiles, wy), dim3(SAL_T), lds, stream, dx, x, perm, sample, baseline, out, M,
                       M, Mp, F, nw, steps, method, absolute ? 1 : 0);
    if (acc) {
        const long long NF = (long long)M * F;
        note_dispatch_more("saliency_class_sum_kernel");
        launch_class_sum(out, cls, acc, nw, NF, ncls, stream);
    }
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}
