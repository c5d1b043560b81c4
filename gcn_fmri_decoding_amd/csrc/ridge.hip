// Cross-validated ridge encoding models (encoding.ridge_cv): every fold's fit and every held-out score of every vertex from three
// per-run statistics -- c_r = Xc_r^T y_r [F][Mp] (chebgcn_glm_project over [Xc_r | 1]), tss_r, and the host's tables of every
// model (V, H, the reciprocals d: include/chebgcn.h) -- without a second pass over the scan and without a [T, M] prediction.
//
// EVERY OPERATION IS A SEPARATE CORRECTLY ROUNDED float64 MULTIPLY, ADD, DIVIDE OR SQUARE ROOT: contraction is off for this file
// (the pragma below), every chain starts from 0 and runs over ascending index, so that encoding.py's NumPy restatement agrees bit
// for bit and a vertex's result does not depend on M, on the other models of the call or on how runs were batched.
//
// All three kernels have one shape: a workgroup of 4 waves owns RG_V = 64 consecutive vertices, LANES OVER VERTICES (plane reads
// and writes coalesce: 512 bytes a wave), and holds one F-vector per vertex in LDS, s[j][lane] (F * 512 bytes: 128 KB at F = 256;
// two such vectors, or a 64-vertex tile of three, do not fit the 160 KB).  The product out_i = sum_j T[j][i] x_j runs in register
// blocks of RG_NI = 16 outputs per lane (ridge_block): per j ONE ds_read_b64 of x_j feeds 16 multiplies and 16 adds, and row j of
// the table, T[j][i0 .. i0 + 16), is the same for every lane -- 128 contiguous bytes through the scalar cache, entering the
// multiplies as scalar operands.  The blocks of 16 are dealt to the four waves.
//
//   ridge_rotate   workgroup (tile, train | test, model): the run sums ct_j (cs_j) into LDS -- wave w the rows j = w, w + 4, ..,
//                  four rows and four runs of loads in flight -- then z = V^T ct (g = V^T cs) block by block into the workspace
//                  [models][2][F][Mp].  The statistics are read ONCE per (model, list); the workspace is written once.
//   ridge_score<FB>  workgroup (tile, fold model), FB in {64, 128, 256} the bucket of F: z into LDS; a wave owns FB / 64 CONSECUTIVE
//                  blocks and keeps their g_i and, per penalty, their h_i = sum_j H[j][i] (d[a][j] z_j) in registers (the scaling is
//                  one more multiply per LDS read; w is never stored).  The chains p = sum_i w_i g_i and q = sum_i w_i h_i run over
//                  ascending i THROUGH the four waves in turn (a handoff of p and q through LDS: 4 barriers a penalty, F
//                  multiply-adds against F^2 / 4 a wave before them).  The last wave forms rss, R^2 or r: float64 [models][A][Mp].
//   ridge_select   thread (subject, vertex): the mean over the subject's folds per penalty, the first maximum, one rounding.
//   ridge_weights  workgroup (tile, subject): t_j = d[a*(m)][j] z_j of the subject's all-runs model into LDS (the reciprocal row is
//                  the lane's own: a gather from a table of at most 64 KB), then w = Vt^T t block by block, rounded once.
// What bounds them: the multiplies and adds of ridge_score, (2 + 2 F) A F float64 instructions per (fold, vertex) and no FMA among
// them -- the bit-for-bit contract with NumPy costs half the vector rate (DESIGN 4.35 has the measured times and the floor).  At
// F > 128 the LDS image leaves one workgroup (one wave per SIMD) a CU: nothing hides the latency of a scalar row behind another
// wave, the row loads are issued ahead by unrolling j.
// Nothing read from memory is an address or a trip count unchecked: list pointers are clamped into [0, nlist], a descending pair
// is an empty list, a list is cut at RG_RUNS entries, a run number outside [0, R) is skipped, fold pointers are clamped into
// [0, E], a model number outside [0, E) gives weights of zero, a selected index is clamped into [0, A).  No float atomics.
#pragma clang fp contract(off)
#include <limits.h>

#include "common.h"

namespace chebgcn {

constexpr int RG_V = 64;                    // vertices of a workgroup: one per lane
constexpr int RG_NW = 4;                    // waves of a workgroup
constexpr int RG_NI = 16;                   // outputs of a register block
constexpr int RG_FMAX = 256;                // features
constexpr int RG_AMAX = 32;                 // penalties
constexpr int RG_RUNS = 64;                 // runs of one list
constexpr int RG_EMAX = 65535;              // models / subjects of one call (grid.z, grid.y)
constexpr int RG_T = 256;                   // threads of ridge_select

static inline int rg_bucket(int F) { return F <= 64 ? 64 : F <= 128 ? 128 : 256; }
static inline size_t rg_lds(int F) { return ((size_t)F * RG_V + 2 * RG_V) * sizeof(double); }

// acc_u = sum_j T[j][i0 + u] * (SCALE ? scale[j] * s[j][lane] : s[j][lane]), u < RG_NI, ONE chain from 0 over ascending j per
// output.  T is [F][F] row-major and wave-uniform, as scale.  FULL: i0 + RG_NI <= F; else the columns beyond F - 1 read column
// F - 1 (in bounds) and the caller drops them
template <bool SCALE, bool FULL>
__device__ __forceinline__ void ridge_block_body(double (&acc)[RG_NI], const double* __restrict__ T, const double* __restrict__ scale,
                                                 int F, int i0, const double* s, int lane) {
#pragma unroll
    for (int u = 0; u < RG_NI; ++u) acc[u] = 0.0;
#pragma unroll 4
    for (int j = 0; j < F; ++j) {
        double x = s[j * RG_V + lane];
        if (SCALE) x = scale[j] * x;
        const double* row = T + (size_t)j * F;
#pragma unroll
        for (int u = 0; u < RG_NI; ++u) {
            const double t = row[FULL ? i0 + u : min(i0 + u, F - 1)];
            acc[u] = acc[u] + t * x;
        }
    }
}

template <bool SCALE>
__device__ __forceinline__ void ridge_block(double (&acc)[RG_NI], const double* __restrict__ T, const double* __restrict__ scale, int F,
                                            int i0, const double* s, int lane) {
    if (i0 + RG_NI <= F) ridge_block_body<SCALE, true>(acc, T, scale, F, i0, s, lane);
    else ridge_block_body<SCALE, false>(acc, T, scale, F, i0, s, lane);
}

// the list `which` of model e: first entry and length, clamped
__device__ __forceinline__ void ridge_list(const int32_t* __restrict__ ptr, int seg, int nlist, int& b, int& n) {
    b = min(max(ptr[seg], 0), nlist);
    const int en = min(max(ptr[seg + 1], 0), nlist);
    n = min(max(en - b, 0), RG_RUNS);
}

// The pointers are kernel arguments of their own, __restrict__: a table read with a wave-uniform address then goes through the
// scalar cache even after the kernel's first store (behind a struct the compiler must assume the store hit the table).
struct RgShape {
    int R, E, F, A, M, Mp, nlist, kind;
};

// block (64 vertices, list blockIdx.y of model blockIdx.z).  c [R][F][Mp]; ptr [2 E + 1]: list 2 e = the training runs of model e,
// 2 e + 1 its held-out runs; runs [nlist]; V [E][F][F] = V[j][i]; ws [E][2][F][Mp]
__global__ void __launch_bounds__(RG_NW * 64)
ridge_rotate_kernel(const double* __restrict__ c_, const int32_t* __restrict__ ptr_, const int32_t* __restrict__ runs_,
                    const double* __restrict__ V_, double* __restrict__ ws_, RgShape p) {
    extern __shared__ __attribute__((aligned(16))) double rg_s[];         // [F][64]
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int e = blockIdx.z, which = blockIdx.y;
    const int m = blockIdx.x * RG_V + lane;
    const bool live = m < p.M;                              // (pad and beyond: the sums are 0, nothing is read)
    const int mm = live ? m : 0;
    const int F = p.F, Mp = p.Mp;
    int b, n;
    ridge_list(ptr_, 2 * e + which, p.nlist, b, n);

    // the run sums: rows j = w, w + 4, ..; four rows a turn, the runs four at a time, every load ahead of its chain
    for (int j0 = w; j0 < F; j0 += 4 * RG_NW) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int u0 = 0; u0 < n; u0 += 4) {
            double v[4][4];
            bool ok[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int run = u0 + u < n ? runs_[b + u0 + u] : -1;
                ok[u] = run >= 0 && run < p.R;
                const int rr = ok[u] ? run : 0;
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const int j = min(j0 + jj * RG_NW, F - 1);
                    v[u][jj] = live ? c_[((size_t)rr * F + j) * Mp + mm] : 0.0;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
                    if (ok[u]) acc[jj] = acc[jj] + v[u][jj];
        }
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int j = j0 + jj * RG_NW;
            if (j < F) rg_s[j * RG_V + lane] = acc[jj];
        }
    }
    __syncthreads();

    const double* __restrict__ V = V_ + (size_t)e * F * F;
    double* __restrict__ out = ws_ + ((size_t)e * 2 + which) * F * Mp;
    const int nb = (F + RG_NI - 1) / RG_NI;
    for (int blk = w; blk < nb; blk += RG_NW) {
        double acc[RG_NI];
        ridge_block<false>(acc, V, nullptr, F, blk * RG_NI, rg_s, lane);
        if (m < Mp) {
#pragma unroll
            for (int u = 0; u < RG_NI; ++u) {
                const int i = blk * RG_NI + u;
                if (i < F) out[(size_t)i * Mp + m] = acc[u];
            }
        }
    }
}

// block (64 vertices, fold model blockIdx.y); PER = FB / 64 the blocks of 16 outputs a wave owns at most.  ws [E][2][F][Mp];
// tss [R][Mp]; ptr / runs as above; H [E][F][F], symmetric bit for bit, read as H[j][i]; d [E][A][F]; fold [Ef][A][Mp]
template <int FB>
__global__ void __launch_bounds__(RG_NW * 64)
ridge_score_kernel(const double* __restrict__ ws_, const double* __restrict__ tss_, const int32_t* __restrict__ ptr_,
                   const int32_t* __restrict__ runs_, const double* __restrict__ H_, const double* __restrict__ d_,
                   double* __restrict__ fold_, RgShape p) {
    constexpr int PER = FB / (RG_NI * RG_NW);
    extern __shared__ __attribute__((aligned(16))) double rg_s[];         // z [F][64], then p [64], q [64]
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int e = blockIdx.y;
    const int m = blockIdx.x * RG_V + lane;
    const bool live = m < p.M;
    const int mm = live ? m : 0;
    const int F = p.F, Mp = p.Mp;
    double* hand = rg_s + F * RG_V;
    const double* __restrict__ z = ws_ + (size_t)e * 2 * F * Mp;
    const double* __restrict__ g = z + (size_t)F * Mp;
    for (int j = w; j < F; j += RG_NW) rg_s[j * RG_V + lane] = live ? z[(size_t)j * Mp + mm] : 0.0;

    // the blocks of this wave: [w per, (w + 1) per) of nb, consecutive, so that the chains below pass through the waves in order
    const int nb = (F + RG_NI - 1) / RG_NI;
    const int per = (nb + RG_NW - 1) / RG_NW;               // (<= PER)
    double gi[PER][RG_NI];
#pragma unroll
    for (int kb = 0; kb < PER; ++kb)
#pragma unroll
        for (int u = 0; u < RG_NI; ++u) {
            const int i = (w * per + kb) * RG_NI + u;
            gi[kb][u] = (live && kb < per && i < F) ? g[(size_t)i * Mp + mm] : 0.0;
        }

    double tss = 0.0;
    if (w == RG_NW - 1) {
        int b, n;
        ridge_list(ptr_, 2 * e + 1, p.nlist, b, n);
        for (int u = 0; u < n; ++u) {
            const int run = runs_[b + u];
            const bool ok = run >= 0 && run < p.R;
            const double v = (ok && live) ? tss_[(size_t)(ok ? run : 0) * Mp + mm] : 0.0;
            if (ok) tss = tss + v;
        }
    }
    __syncthreads();

    for (int a = 0; a < p.A; ++a) {
        const double* __restrict__ da = d_ + ((size_t)e * p.A + a) * F;
        double h[PER][RG_NI];
#pragma unroll
        for (int kb = 0; kb < PER; ++kb) {
            const int blk = w * per + kb;
            if (kb < per && blk < nb) ridge_block<true>(h[kb], H_ + (size_t)e * F * F, da, F, blk * RG_NI, rg_s, lane);
        }
        double pa = 0.0, qa = 0.0;
        for (int ww = 0; ww < RG_NW; ++ww) {
            if (w == ww) {
                if (ww > 0) {
                    pa = hand[lane];
                    qa = hand[RG_V + lane];
                }
#pragma unroll
                for (int kb = 0; kb < PER; ++kb) {
                    const int blk = w * per + kb;
                    if (kb < per && blk < nb) {
#pragma unroll
                        for (int u = 0; u < RG_NI; ++u) {
                            const int i = blk * RG_NI + u;
                            if (i < F) {
                                const double wi = da[i] * rg_s[i * RG_V + lane];
                                pa = pa + wi * gi[kb][u];
                                qa = qa + wi * h[kb][u];
                            }
                        }
                    }
                }
                if (ww < RG_NW - 1) {
                    hand[lane] = pa;
                    hand[RG_V + lane] = qa;
                }
            }
            __syncthreads();
        }
        if (w == RG_NW - 1 && m < Mp) {
            double out;
            if (p.kind == 0) {
                const double rss = (tss - 2.0 * pa) + qa;
                out = tss > 0.0 ? 1.0 - rss / tss : 0.0;
            } else {
                out = (tss > 0.0 && qa > 0.0) ? pa / sqrt(tss * qa) : 0.0;
            }
            fold_[((size_t)e * p.A + a) * Mp + m] = out;
        }
    }
}

// thread (vertex, subject blockIdx.y): fold holds [Ef][A][Mp]
__global__ void __launch_bounds__(RG_T)
ridge_select_kernel(const double* __restrict__ fold, const int32_t* __restrict__ fold_ptr, int Ef, int A, int M, int Mp,
                    float* __restrict__ score, int32_t* __restrict__ index, float* __restrict__ scores) {
    const int m = blockIdx.x * RG_T + threadIdx.x;
    const int s = blockIdx.y;
    if (m >= M) return;
    const int e0 = min(max(fold_ptr[s], 0), Ef);
    const int e1 = min(max(fold_ptr[s + 1], 0), Ef);
    const int n = max(e1 - e0, 0);
    double best = 0.0;
    int ibest = 0;
    for (int a = 0; a < A; ++a) {
        double acc = 0.0;
        for (int e = e0; e < e0 + n; ++e) acc = acc + fold[((size_t)e * A + a) * Mp + m];
        const double mean = n ? acc / (double)n : 0.0;
        if (scores) scores[((size_t)s * A + a) * M + m] = (float)mean;
        if (a == 0 || mean > best) {
            best = mean;
            ibest = a;
        }
    }
    score[(size_t)s * M + m] = (float)best;
    index[(size_t)s * M + m] = ibest;
}

// block (64 vertices, subject blockIdx.y).  ws [E][2][F][Mp]; Vt [E][F][F], Vt[j][i] = V[i][j]; d [E][A][F]; model [S] the all-runs
// model of every subject; index [S][M]; weights [S][F][M]
__global__ void __launch_bounds__(RG_NW * 64)
ridge_weights_kernel(const double* __restrict__ ws_, const double* __restrict__ Vt_, const double* __restrict__ d_,
                     const int32_t* __restrict__ model_, const int32_t* __restrict__ index_, float* __restrict__ weights_, RgShape p) {
    extern __shared__ __attribute__((aligned(16))) double rg_s[];         // t [F][64]
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int s = blockIdx.y;
    const int m = blockIdx.x * RG_V + lane;
    const bool live = m < p.M;
    const int mm = live ? m : 0;
    const int F = p.F, Mp = p.Mp;
    const int e = model_[s];
    const int nb = (F + RG_NI - 1) / RG_NI;
    if (e < 0 || e >= p.E) {                                 // (the same for every thread of the workgroup)
        if (live)
            for (int i = w; i < F; i += RG_NW) weights_[((size_t)s * F + i) * p.M + m] = 0.f;
        return;
    }
    const int a = live ? min(max(index_[(size_t)s * p.M + mm], 0), p.A - 1) : 0;
    const double* __restrict__ z = ws_ + (size_t)e * 2 * F * Mp;
    const double* da = d_ + ((size_t)e * p.A + a) * F;
    for (int j = w; j < F; j += RG_NW) rg_s[j * RG_V + lane] = live ? da[j] * z[(size_t)j * Mp + mm] : 0.0;
    __syncthreads();
    const double* __restrict__ Vt = Vt_ + (size_t)e * F * F;
    for (int blk = w; blk < nb; blk += RG_NW) {
        double acc[RG_NI];
        ridge_block<false>(acc, Vt, nullptr, F, blk * RG_NI, rg_s, lane);
        if (live) {
#pragma unroll
            for (int u = 0; u < RG_NI; ++u) {
                const int i = blk * RG_NI + u;
                if (i < F) weights_[((size_t)s * F + i) * p.M + m] = (float)acc[u];
            }
        }
    }
}

template <int FB>
static int rg_launch_score(const double* ws, const double* tss, const int32_t* ptr, const int32_t* runs, const double* H, const double* d,
                           double* fold, const RgShape& p, int Ef, hipStream_t stream) {
    static char name[40];
    static const int named = snprintf(name, sizeof name, "ridge_score_kernel<%d>", FB);
    (void)named;
    note_dispatch(name);
    const size_t lds = rg_lds(p.F);
    if (lds > 48 * 1024)                        // (an attribute of the function on the current device; no allocation)
        CG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ridge_score_kernel<FB>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
    hipLaunchKernelGGL(ridge_score_kernel<FB>, dim3((unsigned)((p.Mp + RG_V - 1) / RG_V), (unsigned)Ef), dim3(RG_NW * 64), lds, stream, ws, tss,
                       ptr, runs, H, d, fold, p);
    return CHEBGCN_OK;
}

static inline bool rg_shape_ok(int E, int F, int M) { return E >= 1 && F >= 1 && M >= 1 && M <= INT_MAX - 63; }
static inline bool rg_aligned8(const void* q) { return ((uintptr_t)q & 7) == 0; }
static inline bool rg_aligned4(const void* q) { return ((uintptr_t)q & 3) == 0; }
static inline size_t rg_ws_bytes(int E, int F, int M) { return (size_t)E * 2 * (size_t)F * (size_t)plane_stride(M) * sizeof(double); }

}  // namespace chebgcn

using namespace chebgcn;

extern "C" int chebgcn_ridge_query(int what) {
    switch (what) {
        case 0: return RG_V;                // vertices of a workgroup
        case 1: return RG_NI;               // outputs of a register block
        case 2: return RG_FMAX;             // the largest F
        case 3: return RG_AMAX;             // ... number of penalties
        case 4: return RG_RUNS;             // runs of one list
        case 5: return RG_EMAX;             // models / subjects of one call
        case 6: return RG_NW * 64;          // threads of a workgroup
        default: break;
    }
    if (what > 100 && what <= 100 + RG_FMAX) return rg_bucket(what - 100);      // the score kernel's bucket of F
    return -1;
}

extern "C" size_t chebgcn_ridge_workspace(int E, int F, int M) {
    if (!rg_shape_ok(E, F, M) || E > RG_EMAX || F > RG_FMAX) return 0;
    return rg_ws_bytes(E, F, M);
}

extern "C" int chebgcn_ridge_rotate(const double* c, int R, const int32_t* list_ptr, const int32_t* list_runs, int nlist, const double* V,
                                    int E, int F, int M, double* workspace, size_t workspace_bytes, chebgcn_stream stream_) {
    CG_REQUIRE(c && list_ptr && list_runs && V && workspace, "ridge_rotate: NULL argument");
    CG_REQUIRE(rg_shape_ok(E, F, M) && R >= 1 && nlist >= 1, "ridge_rotate: bad shape (R = %d, E = %d, F = %d, M = %d, %d listed runs)", R,
               E, F, M, nlist);
    if (E > RG_EMAX || F > RG_FMAX)
        return fail(CHEBGCN_EUNSUPPORTED, "ridge_rotate: E = %d, F = %d; served: E <= %d, F <= %d", E, F, RG_EMAX, RG_FMAX);
    CG_REQUIRE(workspace_bytes >= rg_ws_bytes(E, F, M), "ridge_rotate: workspace of %zu bytes, %zu needed", workspace_bytes,
               rg_ws_bytes(E, F, M));
    CG_REQUIRE(rg_aligned8(c) && rg_aligned8(V) && rg_aligned8(workspace) && rg_aligned4(list_ptr) && rg_aligned4(list_runs),
               "ridge_rotate: unaligned argument");
    const int Mp = plane_stride(M);
    const RgShape p{R, E, F, 0, M, Mp, nlist, 0};
    const size_t lds = rg_lds(F);
    if (lds > 48 * 1024)
        CG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ridge_rotate_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    note_dispatch("ridge_rotate_kernel");
    hipLaunchKernelGGL(ridge_rotate_kernel, dim3((unsigned)((Mp + RG_V - 1) / RG_V), 2u, (unsigned)E), dim3(RG_NW * 64), lds,
                       (hipStream_t)stream_, c, list_ptr, list_runs, V, workspace, p);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_ridge_score(const double* workspace, size_t workspace_bytes, const double* tss, int R, const int32_t* list_ptr,
                                   const int32_t* list_runs, int nlist, const double* H, const double* d, const int32_t* fold_ptr, int E,
                                   int Ef, int S, int F, int A, int M, int kind, double* fold_scores, float* score, int32_t* alpha_index,
                                   float* scores, chebgcn_stream stream_) {
    CG_REQUIRE(workspace && tss && list_ptr && list_runs && H && d && fold_ptr && fold_scores && score && alpha_index,
               "ridge_score: NULL argument");
    CG_REQUIRE(rg_shape_ok(E, F, M) && R >= 1 && nlist >= 1 && Ef >= 1 && Ef <= E && S >= 1 && A >= 1,
               "ridge_score: bad shape (R = %d, E = %d, Ef = %d, S = %d, F = %d, A = %d, M = %d, %d listed runs)", R, E, Ef, S, F, A, M,
               nlist);
    CG_REQUIRE(kind == CHEBGCN_RIDGE_R2 || kind == CHEBGCN_RIDGE_R, "ridge_score: unknown score %d", kind);
    if (E > RG_EMAX || S > RG_EMAX || F > RG_FMAX || A > RG_AMAX)
        return fail(CHEBGCN_EUNSUPPORTED, "ridge_score: E = %d, S = %d, F = %d, A = %d; served: E, S <= %d, F <= %d, A <= %d", E, S, F, A,
                    RG_EMAX, RG_FMAX, RG_AMAX);
    CG_REQUIRE(workspace_bytes >= rg_ws_bytes(E, F, M), "ridge_score: workspace of %zu bytes, %zu needed", workspace_bytes,
               rg_ws_bytes(E, F, M));
    CG_REQUIRE(rg_aligned8(workspace) && rg_aligned8(tss) && rg_aligned8(H) && rg_aligned8(d) && rg_aligned8(fold_scores) &&
                   rg_aligned4(list_ptr) && rg_aligned4(list_runs) && rg_aligned4(fold_ptr) && rg_aligned4(score) &&
                   rg_aligned4(alpha_index) && rg_aligned4(scores),
               "ridge_score: unaligned argument");
    const int Mp = plane_stride(M);
    const RgShape p{R, E, F, A, M, Mp, nlist, kind};
    hipStream_t stream = (hipStream_t)stream_;
    const int FB = rg_bucket(F);
    const auto launch = FB == 64 ? rg_launch_score<64> : FB == 128 ? rg_launch_score<128> : rg_launch_score<256>;
    const int rc = launch(workspace, tss, list_ptr, list_runs, H, d, fold_scores, p, Ef, stream);
    if (rc != CHEBGCN_OK) return rc;
    note_dispatch_more("ridge_select_kernel");
    hipLaunchKernelGGL(ridge_select_kernel, dim3((unsigned)((M + RG_T - 1) / RG_T), (unsigned)S), dim3(RG_T), 0, stream, fold_scores,
                       fold_ptr, Ef, A, M, Mp, score, alpha_index, scores);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_ridge_weights(const double* workspace, size_t workspace_bytes, const double* Vt, const double* d,
                                     const int32_t* all_model, const int32_t* alpha_index, int E, int S, int F, int A, int M,
                                     float* weights, chebgcn_stream stream_) {
    CG_REQUIRE(workspace && Vt && d && all_model && alpha_index && weights, "ridge_weights: NULL argument");
    CG_REQUIRE(rg_shape_ok(E, F, M) && S >= 1 && A >= 1, "ridge_weights: bad shape (E = %d, S = %d, F = %d, A = %d, M = %d)", E, S, F, A, M);
    if (E > RG_EMAX || S > RG_EMAX || F > RG_FMAX || A > RG_AMAX)
        return fail(CHEBGCN_EUNSUPPORTED, "ridge_weights: E = %d, S = %d, F = %d, A = %d; served: E, S <= %d, F <= %d, A <= %d", E, S, F, A,
                    RG_EMAX, RG_FMAX, RG_AMAX);
    CG_REQUIRE(workspace_bytes >= rg_ws_bytes(E, F, M), "ridge_weights: workspace of %zu bytes, %zu needed", workspace_bytes,
               rg_ws_bytes(E, F, M));
    CG_REQUIRE(rg_aligned8(workspace) && rg_aligned8(Vt) && rg_aligned8(d) && rg_aligned4(all_model) && rg_aligned4(alpha_index) &&
                   rg_aligned4(weights),
               "ridge_weights: unaligned argument");
    const int Mp = plane_stride(M);
    const RgShape p{0, E, F, A, M, Mp, 0, 0};
    const size_t lds = rg_lds(F);
    if (lds > 48 * 1024)
        CG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ridge_weights_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    note_dispatch("ridge_weights_kernel");
    hipLaunchKernelGGL(ridge_weights_kernel, dim3((unsigned)((M + RG_V - 1) / RG_V), (unsigned)S), dim3(RG_NW * 64), lds,
                       (hipStream_t)stream_, workspace, Vt, d, all_model, alpha_index, weights, p);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}
