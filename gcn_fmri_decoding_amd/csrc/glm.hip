// First-level general linear model on staged scans (glm.first_level): per run and vertex the least-squares fit of a design, its
// residual variance, and contrast effects, variances and t values -- without ever forming the residual series.
//
// The host hands every run its design as an orthonormal basis: X = U S V^T (thin SVD, rank k), Q = U[:, :k].  Then
//     a = Q^T y                 the projections: the only pass over the scan (glm_project)
//     rss = y.y - a.a           the residual sum of squares, by Pythagoras
//     b = B a, B = V / S        the minimum-norm coefficients
//     c.b = u.a, u = B^T c      a contrast's effect;  c pinv(X^T X) c = u.u  its variance factor
// Everything is float64: on BOLD-scaled data (mean 1e4, noise sd 50) rss is 2e-5 of y.y, and a float32 sum of y.y or of a
// projection is off by more than that difference.
//
//   glm_project<NJ>  workgroup (run, 128 vertices), 4 waves: a lane owns TWO consecutive vertices (one 8-byte load per row) and
//                    2 NJ float64 accumulators (4 NJ VGPRs) + 2 for y.y; rows are read coalesced, vertex fastest, four rows in
//                    flight while the four before them are worked on -- no load stands behind a branch, or the compiler waits
//                    for each one at the join (measured: 0.175 ms instead of 0.077 ms for the bare pass over 438 MB).
//                    A row of Q is the same for every lane: it comes through the scalar cache (the address is a function of the
//                    run, the wave and the loop counter alone) and enters the FMA as a scalar operand -- through LDS a broadcast
//                    read would cost as many cycles as the FMA it feeds, for all four SIMDs at once.  Two vertices per lane
//                    halve the scalar bytes per FMA.  k > 16 runs in column panels of 16 (the last one narrower: exactly its
//                    columns, no FMA on padding), the scan re-read per panel, y.y summed in the first: a row of more than 16
//                    columns takes more than a third of a wave's SGPRs, the next row's scalar load can no longer be in flight
//                    during the FMAs of this one, and a pass costs more than two narrower ones (measured).
//                    The time loop of a run of T >= GLM_SPLIT rows is cut into n = min(4, T / GLM_SLICE) slices of ceil(T / n)
//                    rows, one per wave -- a function of T ALONE; the slices' sums are added to wave 0's in ascending order
//                    through LDS.  Shorter runs are wave 0's alone.  So a (run, vertex) result is the same bits whatever else the
//                    call holds, however the caller batches runs, whatever M is.
//   glm_finish       thread (run, vertex): a.a in ascending j, rss with its round-off floor, sigma^2, then per contrast u.a in
//                    ascending j; optionally b = B a.  a is re-read per contrast (coalesced, from L2); u and B rows are scalar.
//   glm_combine      thread (group, contrast, vertex): float64 sums over the group's runs in the order of its list.
// No float atomics anywhere.  Nothing read from memory is an address or a trip count unchecked: run offsets are clamped into
// [0, Ttot], ranks into [0, k], run numbers of a group are skipped when outside [0, R).
#include <limits.h>

#include <utility>

#include "common.h"

namespace chebgcn {

#ifndef CG_GLM_V
#define CG_GLM_V 2
#endif
#ifndef CG_GLM_PANEL
#define CG_GLM_PANEL 16
#endif
#ifndef CG_GLM_U
#define CG_GLM_U 4
#endif
constexpr int GLM_U = CG_GLM_U;             // rows of a lane in flight
constexpr int GLM_V = CG_GLM_V;             // consecutive vertices of a lane
constexpr int GLM_VB = 64 * GLM_V;          // vertices of a project workgroup
constexpr int GLM_NW = 4;                   // its waves: slices of the time loop
constexpr int GLM_PANEL = CG_GLM_PANEL;     // columns of Q of one pass over the scan: a lane holds GLM_V * GLM_PANEL accumulators
constexpr int GLM_KMAX = 64;                // rank of a design
constexpr int GLM_CMAX = 32;                // contrasts
constexpr int GLM_PMAX = 64;                // columns of a design (rows of B)
constexpr int GLM_SLICE = 32;               // a wave's slice is at least this many rows
constexpr int GLM_SPLIT = 2 * GLM_SLICE;    // runs from this length are split
constexpr int GLM_T = 256;                  // threads of finish / combine
constexpr int GLM_RMAX = 65535;             // runs of one call (grid.y)
constexpr int GLM_SMAX = 65535;             // groups of one call (grid.z)
constexpr long long GLM_ELEMS = 0x7fffffffffLL;   // Ttot * Mp at most

// rows [t0, t1) of run r inside [0, Ttot]; a descending pair is an empty run
__device__ __forceinline__ void glm_run(const long long* __restrict__ offs, int r, long long Ttot, long long& t0, long long& t1) {
    t0 = min(max(offs[r], 0LL), Ttot);
    t1 = min(max(offs[r + 1], t0), Ttot);
}

template <int V, int NJ>
__device__ __forceinline__ void glm_row(double (&acc)[V][NJ], double (&q2)[V], const float (&y)[V], const double* __restrict__ q,
                                        bool first) {
    double yd[V];
#pragma unroll
    for (int v = 0; v < V; ++v) yd[v] = (double)y[v];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const double qj = q[j];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v][j] = fma(qj, yd[v], acc[v][j]);
    }
    if (first) {
#pragma unroll
        for (int v = 0; v < V; ++v) q2[v] = fma(yd[v], yd[v], q2[v]);
    }
}

// the V values of a lane in one row; a pad column (and a vector beyond Mp) gives 0 whatever the memory holds.  No branch: a lane
// beyond the row reads the row's first vector and drops it, so the loads of several rows stay in flight together
template <int V>
__device__ __forceinline__ void glm_load(float (&y)[V], const float* __restrict__ row, int m0, int M, int Mp) {
    typedef float vec __attribute__((ext_vector_type(V)));
    const vec x = *reinterpret_cast<const vec*>(row + (m0 < Mp ? m0 : 0));
#pragma unroll
    for (int v = 0; v < V; ++v) y[v] = m0 + v < M ? x[v] : 0.f;
}
template <>
__device__ __forceinline__ void glm_load<1>(float (&y)[1], const float* __restrict__ row, int m0, int M, int Mp) {
    const float x = row[m0 < Mp ? m0 : 0];
    y[0] = m0 < M ? x : 0.f;
}

// block (GLM_VB vertices, run blockIdx.y), 4 waves; columns [j0, j0 + NJ) of Q, j0 + NJ <= k
template <int V, int NJ>
__global__ void __launch_bounds__(GLM_NW * 64)
glm_project_kernel(const float* __restrict__ series, long long Ttot, const long long* __restrict__ offs, int M, int Mp,
                   const double* __restrict__ Q, int k, int j0, double* __restrict__ a, double* __restrict__ yy) {
    __shared__ double red[V * (NJ + 1) * 64];
    const int r = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m0 = blockIdx.x * (64 * V) + lane * V;        // (Mp is a multiple of 32: a vector is inside the row or beyond it)
    const bool first = j0 == 0;
    long long t0, t1;
    glm_run(offs, r, Ttot, t0, t1);
    const long long T = t1 - t0;
    const int nsl = T < GLM_SPLIT ? 1 : (int)min((long long)GLM_NW, T / GLM_SLICE);
    const long long len = (T + nsl - 1) / nsl;
    const long long ta = min(t0 + (long long)w * len, t1), tb = w < nsl ? min(ta + len, t1) : ta;

    double acc[V][NJ], q2[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        q2[v] = 0.0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[v][j] = 0.0;
    }
    // GLM_U rows in flight while the GLM_U before them are worked on.  No load stands behind a branch (the compiler would wait for
    // each one at the join): a row at or beyond tb is read as row tb - 1 and never used
    if (ta < tb) {
        float cur[GLM_U][V], nxt[GLM_U][V];
#pragma unroll
        for (int u = 0; u < GLM_U; ++u) glm_load<V>(cur[u], series + (size_t)min(ta + u, tb - 1) * Mp, m0, M, Mp);
        for (long long t = ta; t < tb; t += GLM_U) {
#pragma unroll
            for (int u = 0; u < GLM_U; ++u) glm_load<V>(nxt[u], series + (size_t)min(t + GLM_U + u, tb - 1) * Mp, m0, M, Mp);
            if (t + GLM_U <= tb) {
#pragma unroll
                for (int u = 0; u < GLM_U; ++u) glm_row<V, NJ>(acc, q2, cur[u], Q + (size_t)(t + u) * k + j0, first);
            } else {
#pragma unroll
                for (int u = 0; u < GLM_U; ++u)
                    if (t + u < tb) glm_row<V, NJ>(acc, q2, cur[u], Q + (size_t)(t + u) * k + j0, first);
            }
#pragma unroll
            for (int u = 0; u < GLM_U; ++u)
#pragma unroll
                for (int v = 0; v < V; ++v) cur[u][v] = nxt[u][v];
        }
    }

    for (int ww = 1; ww < nsl; ++ww) {      // (nsl is the same in every thread)
        if (w == ww) {
#pragma unroll
            for (int v = 0; v < V; ++v) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) red[(v * (NJ + 1) + j) * 64 + lane] = acc[v][j];
                red[(v * (NJ + 1) + NJ) * 64 + lane] = q2[v];
            }
        }
        __syncthreads();
        if (w == 0) {
#pragma unroll
            for (int v = 0; v < V; ++v) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[v][j] = acc[v][j] + red[(v * (NJ + 1) + j) * 64 + lane];
                q2[v] = q2[v] + red[(v * (NJ + 1) + NJ) * 64 + lane];
            }
        }
        __syncthreads();
    }
    if (w != 0 || m0 >= Mp) return;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int v = 0; v < V; ++v) a[((size_t)r * k + j0 + j) * Mp + m0 + v] = acc[v][j];
    if (first)
#pragma unroll
        for (int v = 0; v < V; ++v) yy[(size_t)r * Mp + m0 + v] = q2[v];
}

struct GlmFinish {
    const double* a;            // [R][k][Mp]
    const double* yy;           // [R][Mp]
    const long long* offs;      // [R + 1]
    long long Ttot;
    const int32_t* rank;        // [R]
    const double* U;            // [R][C][k]
    const double* un2;          // [R][C]
    const double* B;            // [R][P][k] or NULL
    double* eff64;              // [R][C][Mp] or NULL
    double* var64;
    float* effect;              // [R][C][Mp] or NULL
    float* variance;
    float* t;
    float* beta;                // [R][P][Mp] or NULL
    int M, Mp, k, C, P;
};

// block (256 vertices, run blockIdx.y)
__global__ void __launch_bounds__(GLM_T)
glm_finish_kernel(GlmFinish p) {
    const int m = blockIdx.x * GLM_T + threadIdx.x;
    const int r = blockIdx.y;
    if (m >= p.Mp) return;
    long long t0, t1;
    glm_run(p.offs, r, p.Ttot, t0, t1);
    const long long T = t1 - t0;
    const int kr = min(max(p.rank[r], 0), p.k);
    const long long dof = T - kr;
    const double* ar = p.a + (size_t)r * p.k * p.Mp + m;
    double ssq = 0.0;
    for (int j = 0; j < kr; ++j) {
        const double v = ar[(size_t)j * p.Mp];
        ssq = fma(v, v, ssq);
    }
    const double y2 = p.yy[(size_t)r * p.Mp + m];
    double rss = y2 - ssq;
    if (rss < 4.0 * (double)(T + kr) * 0x1p-53 * y2) rss = 0.0;      // round-off of the subtraction (also a negative one)
    const double s2 = dof > 0 ? rss / (double)dof : 0.0;
    for (int c = 0; c < p.C; ++c) {
        const double* u = p.U + ((size_t)r * p.C + c) * p.k;
        double e = 0.0;
        for (int j = 0; j < kr; ++j) e = fma(u[j], ar[(size_t)j * p.Mp], e);
        const double v = s2 * p.un2[(size_t)r * p.C + c];
        const double tv = v > 0.0 ? e / sqrt(v) : 0.0;
        const size_t o = ((size_t)r * p.C + c) * p.Mp + m;
        if (p.eff64) p.eff64[o] = e;
        if (p.var64) p.var64[o] = v;
        if (p.effect) p.effect[o] = (float)e;
        if (p.variance) p.variance[o] = (float)v;
        if (p.t) p.t[o] = (float)tv;
    }
    if (p.beta)
        for (int i = 0; i < p.P; ++i) {
            const double* b = p.B + ((size_t)r * p.P + i) * p.k;
            double s = 0.0;
            for (int j = 0; j < kr; ++j) s = fma(b[j], ar[(size_t)j * p.Mp], s);
            p.beta[((size_t)r * p.P + i) * p.Mp + m] = (float)s;
        }
}

// block (256 vertices, contrast blockIdx.y, group blockIdx.z)
__global__ void __launch_bounds__(GLM_T)
glm_combine_kernel(const double* __restrict__ eff64, const double* __restrict__ var64, const int32_t* __restrict__ gptr,
                   const int32_t* __restrict__ gruns, int nruns, int R, int C, int M, int Mp, float* __restrict__ effect,
                   float* __restrict__ variance, float* __restrict__ t) {
    const int m = blockIdx.x * GLM_T + threadIdx.x;
    const int c = blockIdx.y, g = blockIdx.z;
    if (m >= M) return;
    const int i0 = min(max(gptr[g], 0), nruns), i1 = min(max(gptr[g + 1], i0), nruns);
    double se = 0.0, sv = 0.0;
    int n = 0;
    for (int i = i0; i < i1; ++i) {
        const int r = gruns[i];
        if ((unsigned)r >= (unsigned)R) continue;
        const size_t o = ((size_t)r * C + c) * Mp + m;
        se = se + eff64[o];
        sv = sv + var64[o];
        ++n;
    }
    const double e = n ? se / (double)n : 0.0;
    const double v = n ? sv / ((double)n * (double)n) : 0.0;
    const size_t o = ((size_t)g * C + c) * M + m;
    effect[o] = (float)e;
    variance[o] = (float)v;
    t[o] = (float)(v > 0.0 ? e / sqrt(v) : 0.0);
}

// the launch of one panel of NJ columns; names have static storage
template <int NJ>
static int glm_launch_panel(bool more, const float* series, long long Ttot, const long long* offs, int R, int M, int Mp, const double* Q,
                            int k, int j0, double* a, double* yy, hipStream_t stream) {
    static char name[40];
    static const int named = snprintf(name, sizeof name, "glm_project_kernel<%d>", NJ);
    (void)named;
    if (more) note_dispatch_more(name);
    else note_dispatch(name);
    const dim3 grid((unsigned)((Mp + GLM_VB - 1) / GLM_VB), (unsigned)R);
    hipLaunchKernelGGL((glm_project_kernel<GLM_V, NJ>), grid, dim3(GLM_NW * 64), 0, stream, series, Ttot, offs, M, Mp, Q, k, j0, a, yy);
    return CHEBGCN_OK;
}

typedef int (*GlmPanel)(bool, const float*, long long, const long long*, int, int, int, const double*, int, int, double*, double*,
                        hipStream_t);
template <int... NJ>
static GlmPanel glm_panel_of(int nj, std::integer_sequence<int, NJ...>) {
    static const GlmPanel table[] = {glm_launch_panel<NJ + 1>...};
    return table[nj - 1];
}

static inline bool glm_shape_ok(int R, int M) { return R >= 1 && M >= 1; }

}  // namespace chebgcn

using namespace chebgcn;

extern "C" int chebgcn_glm_query(int what) {
    switch (what) {
        case 0: return GLM_VB;              // vertices of a project workgroup
        case 1: return GLM_PANEL;           // columns of Q of one pass over the scan
        case 2: return GLM_KMAX;            // the largest rank
        case 3: return GLM_CMAX;            // ... number of contrasts
        case 4: return GLM_SPLIT;           // run length from which the time loop is split
        case 5: return GLM_SLICE;           // least rows of a slice
        case 6: return GLM_NW;              // slices at most
        case 7: return GLM_PMAX;            // the largest number of design columns (rows of B)
        case 8: return GLM_RMAX;            // runs of one call
        default: return -1;
    }
}

extern "C" size_t chebgcn_glm_workspace(int R, int M, int k) {
    if (!glm_shape_ok(R, M) || R > GLM_RMAX || k < 1 || k > GLM_KMAX || M > INT_MAX - 31) return 0;
    return (size_t)R * (size_t)(k + 1) * (size_t)plane_stride(M) * sizeof(double);
}

extern "C" int chebgcn_glm_project(const float* series, int64_t Ttot, const int64_t* run_offsets, int R, int M, const double* Q, int k,
                                   double* a, double* yy, chebgcn_stream stream_) {
    CG_REQUIRE(series && run_offsets && Q && a && yy, "glm_project: NULL argument");
    CG_REQUIRE(Ttot >= 1 && glm_shape_ok(R, M) && k >= 1 && M <= INT_MAX - 31, "glm_project: bad shape (Ttot = %lld, R = %d, M = %d, k = %d)",
               (long long)Ttot, R, M, k);
    const int Mp = plane_stride(M);
    if (k > GLM_KMAX || R > GLM_RMAX || Ttot > GLM_ELEMS / Mp)
        return fail(CHEBGCN_EUNSUPPORTED, "glm_project: k = %d, R = %d, Ttot = %lld; served: k <= %d, R <= %d, Ttot * Mp <= 2^39", k, R,
                    (long long)Ttot, GLM_KMAX, GLM_RMAX);
    CG_REQUIRE((((uintptr_t)series | (uintptr_t)run_offsets | (uintptr_t)Q | (uintptr_t)a | (uintptr_t)yy) & 7) == 0,
               "glm_project: unaligned argument (8 bytes, series included: a lane loads two vertices at once)");
    for (int j0 = 0; j0 < k; j0 += GLM_PANEL) {
        const int nj = k - j0 < GLM_PANEL ? k - j0 : GLM_PANEL;
        glm_panel_of(nj, std::make_integer_sequence<int, GLM_PANEL>())(j0 > 0, series, (long long)Ttot, (const long long*)run_offsets, R,
                                                                      M, Mp, Q, k, j0, a, yy, (hipStream_t)stream_);
    }
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_glm_finish(const double* a, const double* yy, const int64_t* run_offsets, int64_t Ttot, const int32_t* rank,
                                  const double* U, const double* unorm2, const double* B, int R, int M, int k, int C, int P,
                                  double* eff64, double* var64, float* effect, float* variance, float* t, float* beta,
                                  chebgcn_stream stream_) {
    CG_REQUIRE(a && yy && run_offsets && rank && U && unorm2, "glm_finish: NULL argument");
    CG_REQUIRE((eff64 && var64) || (effect && variance && t) || beta, "glm_finish: no output");
    CG_REQUIRE(!eff64 == !var64 && !effect == !variance && !effect == !t, "glm_finish: effect, variance (and t) come together");
    CG_REQUIRE(!beta == !B, "glm_finish: beta and B come together");
    CG_REQUIRE(Ttot >= 1 && glm_shape_ok(R, M) && k >= 1 && C >= 1 && P >= 0 && (P >= 1 || !beta) && M <= INT_MAX - 31,
               "glm_finish: bad shape (Ttot = %lld, R = %d, M = %d, k = %d, C = %d, P = %d)", (long long)Ttot, R, M, k, C, P);
    if (k > GLM_KMAX || C > GLM_CMAX || P > GLM_PMAX || R > GLM_RMAX)
        return fail(CHEBGCN_EUNSUPPORTED, "glm_finish: k = %d, C = %d, P = %d, R = %d; served: k <= %d, C <= %d, P <= %d, R <= %d", k, C,
                    P, R, GLM_KMAX, GLM_CMAX, GLM_PMAX, GLM_RMAX);
    CG_REQUIRE((((uintptr_t)a | (uintptr_t)yy | (uintptr_t)run_offsets | (uintptr_t)U | (uintptr_t)unorm2 | (uintptr_t)B |
                 (uintptr_t)eff64 | (uintptr_t)var64) & 7) == 0 &&
                   (((uintptr_t)rank | (uintptr_t)effect | (uintptr_t)variance | (uintptr_t)t | (uintptr_t)beta) & 3) == 0,
               "glm_finish: unaligned argument");
    const int Mp = plane_stride(M);
    GlmFinish p{a, yy, (const long long*)run_offsets, (long long)Ttot, rank, U, unorm2, B, eff64, var64, effect, variance, t, beta, M, Mp,
                k, C, P};
    note_dispatch("glm_finish_kernel");
    hipLaunchKernelGGL(glm_finish_kernel, dim3((unsigned)((Mp + GLM_T - 1) / GLM_T), (unsigned)R), dim3(GLM_T), 0, (hipStream_t)stream_, p);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_glm_combine(const double* eff64, const double* var64, const int32_t* group_ptr, const int32_t* group_runs,
                                   int nruns, int R, int S, int C, int M, float* effect, float* variance, float* t,
                                   chebgcn_stream stream_) {
    CG_REQUIRE(eff64 && var64 && group_ptr && group_runs && effect && variance && t, "glm_combine: NULL argument");
    CG_REQUIRE(glm_shape_ok(R, M) && S >= 1 && C >= 1 && nruns >= 1 && M <= INT_MAX - 31,
               "glm_combine: bad shape (R = %d, S = %d, C = %d, M = %d, %d listed runs)", R, S, C, M, nruns);
    if (C > GLM_CMAX || S > GLM_SMAX)
        return fail(CHEBGCN_EUNSUPPORTED, "glm_combine: C = %d, S = %d; served: C <= %d, S <= %d", C, S, GLM_CMAX, GLM_SMAX);
    CG_REQUIRE((((uintptr_t)eff64 | (uintptr_t)var64) & 7) == 0 &&
                   (((uintptr_t)group_ptr | (uintptr_t)group_runs | (uintptr_t)effect | (uintptr_t)variance | (uintptr_t)t) & 3) == 0,
               "glm_combine: unaligned argument");
    note_dispatch("glm_combine_kernel");
    hipLaunchKernelGGL(glm_combine_kernel, dim3((unsigned)((M + GLM_T - 1) / GLM_T), (unsigned)C, (unsigned)S), dim3(GLM_T), 0,
                       (hipStream_t)stream_, eff64, var64, group_ptr, group_runs, nruns, R, C, M, plane_stride(M), effect, variance, t);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}
