// Single-trial patterns by "least squares - separate" (glm.single_trial): per run one GLM per TRIAL j, [x_j | others | N] -- the
// trial's own regressor, the other trials lumped per condition (or into one column), the nuisance columns -- and the trial's
// pattern is the coefficient (or t value) of x_j.  The models of a run differ by one column swap, so one set of projections
// serves them all.  With Qn an orthonormal basis of N (rank q), S the G per-condition sums of the trial columns and
// Z = (I - Qn Qn^T) [X | S], the host hands
//     glm_project over [Qn | Z_S]   an = Qn^T y, c = Z_S^T y, y.y          (the existing kernel: k = q + G columns)
//     glm_trials over Z_X           p_j = z_j^T y, the pass of glm_pass.h over panels of GLM_PANEL trial columns
// and per trial the vertex-independent tables of H_j = D_j^T (I - Qn Qn^T) D_j, D_j = [x_j | S_g - [g = own_j] x_j]: w_j the first
// row of H_j^+, r_j its rank, F_j with F_j^T F_j = H_j^+ (rows >= r_j zero).  Then, float64, every chain in ascending order:
//     d = (p_j, c_g - [g = own_j] p_j);   beta = w_j . d;   ssq = chain of an_i^2, i < q, then of (F_j d)_i^2, i < r_j;
//     rss = y.y - ssq (0 below glm_finish's floor);   variance = rss / (T - q - r_j) * w_j0;   t = beta / sqrt(variance).
//
//   glm_trials<NJ>   the workgroup of glm_project_kernel, with a fused epilogue: the projections are never written out (8 n Mp bytes
//                    per run, more than the outputs themselves).  Wave 0, which holds the sums of the run after the pass, takes
//                    the run's common sums for its vertices from L2 -- the chain of an_i^2 once per vertex: it is the same prefix
//                    for every trial -- and parks them, with its NJ projections, in LDS, one slot per (sum, vertex, lane): G up
//                    to 15 costs the time loop no register.  After one barrier the trials of the panel go round the four waves
//                    (measured: 0.52 ms against 0.63 ms with wave 0 finishing all sixteen).  The trial's own, r_j,
//                    w_j and F_j are the same for every lane: they come through the scalar cache.
//                    The full panels of a call are grid.z of one launch (measured: 0.56 ms against 0.83 ms for a launch per
//                    panel), the last, narrower panel a launch of its own; a run with no trial in a panel leaves at once, a
//                    run with fewer than NJ runs the pass over zero columns of Z and stores only its own.
// No float atomics.  Nothing read from memory is an address or a trip count unchecked: run and trial offsets are clamped into
// range, q_rank into [0, k - G], own into [-1, G), a trial's rank into [0, G1].
#include <limits.h>

#include <utility>

#include "common.h"
#include "glm_pass.h"

namespace chebgcn {

constexpr int GLM_TRIALS_G1 = 16;           // columns of a trial's model besides the nuisance: itself and G <= 15 others
constexpr int GLM_TRIALS_NMAX = 4096;       // trials of one run
#ifndef CG_GLM_TRIALS_Z
#define CG_GLM_TRIALS_Z 1                   // 1: the full panels of a call in grid.z of ONE launch; 0: a launch per panel
#endif

struct GlmTrials {
    const float* series;        // [Ttot][Mp]
    long long Ttot;
    const long long* offs;      // [R + 1]
    const double* Z;            // [Ttot][nmax]
    const long long* toffs;     // [R + 1]
    const double* a;            // [R][k][Mp]: of run r the planes [0, q_r) = an, [q_r, q_r + G) = c
    const double* yy;           // [R][Mp]
    const int32_t* qrank;       // [R]
    const int32_t* own;         // [N]
    const int32_t* rank;        // [N]
    const double* w;            // [N][G1]
    const double* F;            // [N][G1][G1]
    float* beta;                // [N][Mp] or NULL
    float* variance;
    float* t;
    long long N;
    int M, Mp, nmax, k, G1;
};

// One trial of V vertices of a lane: i its row of the flat tables and of the outputs, pj its projections, c the lane's common
// sums in LDS (sum g of vertex v at c[(g * V + v) * 64]), ssn the chain of an^2 so far, y2 = y.y
template <int V>
__device__ __forceinline__ void glm_trial_finish(const GlmTrials& p, size_t i, const double (&pj)[V], const double* c, const double (&ssn)[V],
                                                 const double (&y2)[V], long long T, int qr, int G1, int m0) {
    typedef float vec __attribute__((ext_vector_type(V)));
    const int G = G1 - 1;
    const int own = min(max(p.own[i], -1), G - 1);
    const int rj = min(max(p.rank[i], 0), G1);
    const double* wj = p.w + i * G1;
    const double* Fj = p.F + i * G1 * G1;
    const double w0 = wj[0];
    double b[V], ssq[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        b[v] = fma(w0, pj[v], 0.0);
        ssq[v] = ssn[v];
    }
    for (int l = 1; l < G1; ++l) {
        const double wl = wj[l];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const double d = c[((l - 1) * V + v) * 64] - (l - 1 == own ? pj[v] : 0.0);
            b[v] = fma(wl, d, b[v]);
        }
    }
    for (int i2 = 0; i2 < rj; ++i2) {
        const double* f = Fj + i2 * G1;
        const double f0 = f[0];
        double s[V];
#pragma unroll
        for (int v = 0; v < V; ++v) s[v] = fma(f0, pj[v], 0.0);
        for (int l = 1; l < G1; ++l) {
            const double fl = f[l];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const double d = c[((l - 1) * V + v) * 64] - (l - 1 == own ? pj[v] : 0.0);
                s[v] = fma(fl, d, s[v]);
            }
        }
#pragma unroll
        for (int v = 0; v < V; ++v) ssq[v] = fma(s[v], s[v], ssq[v]);
    }
    const long long dof = T - qr - rj;
    vec ob, ov, ot;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        double rss = y2[v] - ssq[v];
        if (rss < 4.0 * (double)(T + qr + rj) * 0x1p-53 * y2[v]) rss = 0.0;       // round-off of the subtraction (also a negative one)
        const double s2 = dof > 0 ? rss / (double)dof : 0.0;
        const double var = s2 * w0;
        const double tv = var > 0.0 ? b[v] / sqrt(var) : 0.0;
        const bool live = m0 + v < p.M;         // the pad columns of the outputs are zero whatever the planes hold
        ob[v] = live ? (float)b[v] : 0.f;
        ov[v] = live ? (float)var : 0.f;
        ot[v] = live ? (float)tv : 0.f;
    }
    const size_t o = i * (size_t)p.Mp + m0;
    if (p.beta) *reinterpret_cast<vec*>(p.beta + o) = ob;
    if (p.variance) *reinterpret_cast<vec*>(p.variance + o) = ov;
    if (p.t) *reinterpret_cast<vec*>(p.t + o) = ot;
}

// block (GLM_VB vertices, run blockIdx.y, panel blockIdx.z), 4 waves; trial columns [j0, j0 + NJ) of the run, j0 = first + NJ
// blockIdx.z, j0 + NJ <= nmax
template <int V, int NJ>
__global__ void __launch_bounds__(GLM_NW * 64)
glm_trials_kernel(GlmTrials p, int first) {
    const int j0 = first + NJ * (int)blockIdx.z;
    constexpr int GS = GLM_TRIALS_G1 - 1;       // LDS: NJ projections (the pass's sums before), GS common sums, ssn, y.y
    constexpr int LDS = V * (NJ + GS + 2) * 64;
    static_assert(LDS >= glm_pass_lds<V, NJ, false>(), "the pass reduces through the same LDS");
    __shared__ double red[LDS];
    const int r = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m0 = blockIdx.x * (64 * V) + lane * V;
    const int M = p.M, Mp = p.Mp;
    const long long i0 = min(max(p.toffs[r], 0LL), p.N), i1 = min(max(p.toffs[r + 1], i0), p.N);
    const int nr = (int)min(i1 - i0, (long long)p.nmax);
    if (j0 >= nr) return;                       // (the same in every thread of the workgroup)
    long long t0, t1;
    glm_run(p.offs, r, p.Ttot, t0, t1);

    double acc[V][NJ], q2[V], lag[V];
    glm_pass<V, NJ, false, false>(acc, q2, lag, p.series, t0, t1, m0, M, Mp, p.Z, p.nmax, j0, w, lane, red);

    const int G1 = min(max(p.G1, 1), GLM_TRIALS_G1), G = G1 - 1;
    const int qr = min(max(p.qrank[r], 0), p.k - G);
    const long long T = t1 - t0;
    double* cs = red + V * NJ * 64 + lane;
    double* sy = red + V * (NJ + GS) * 64 + lane;
    if (w == 0 && m0 < Mp) {
        const double* ar = p.a + (size_t)r * p.k * Mp + m0;
        double ssn[V];
#pragma unroll
        for (int v = 0; v < V; ++v) ssn[v] = 0.0;
        for (int i = 0; i < qr; ++i) {
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const double x = ar[(size_t)i * Mp + v];
                ssn[v] = fma(x, x, ssn[v]);
            }
        }
        for (int g = 0; g < G; ++g) {
#pragma unroll
            for (int v = 0; v < V; ++v) cs[(g * V + v) * 64] = ar[(size_t)(qr + g) * Mp + v];
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            sy[v * 64] = ssn[v];
            sy[(V + v) * 64] = p.yy[(size_t)r * Mp + m0 + v];
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int v = 0; v < V; ++v) red[(j * V + v) * 64 + lane] = acc[v][j];
    }
    // the trials of the panel go round the waves: a trial's epilogue is two float64 divisions and a square root per vertex behind
    // scalar loads, about as long as a wave's share of the pass, and wave 0 alone would do sixteen of them while three SIMDs idle
    __syncthreads();
    if (m0 >= Mp) return;
    double ssn[V], y2[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        ssn[v] = sy[v * 64];
        y2[v] = sy[(V + v) * 64];
    }
    for (int j = w; j < NJ && j0 + j < nr; j += GLM_NW) {
        double pj[V];
#pragma unroll
        for (int v = 0; v < V; ++v) pj[v] = red[(j * V + v) * 64 + lane];
        glm_trial_finish<V>(p, (size_t)(i0 + j0 + j), pj, cs, ssn, y2, T, qr, G1, m0);
    }
}

// the launch of nz panels of NJ trial columns each, from column j0; names have static storage, one per panel
template <int NJ>
static void glm_trials_launch_panel(bool more, const GlmTrials& p, int R, int j0, int nz, hipStream_t stream) {
    static char name[40];
    static const int named = snprintf(name, sizeof name, "glm_trials_kernel<%d>", NJ);
    (void)named;
    for (int z = 0; z < nz; ++z) {
        if (more || z) note_dispatch_more(name);
        else note_dispatch(name);
    }
    const dim3 grid((unsigned)((p.Mp + GLM_VB - 1) / GLM_VB), (unsigned)R, (unsigned)nz);
    hipLaunchKernelGGL((glm_trials_kernel<GLM_V, NJ>), grid, dim3(GLM_NW * 64), 0, stream, p, j0);
}

typedef void (*GlmTrialsPanel)(bool, const GlmTrials&, int, int, int, hipStream_t);
template <int... NJ>
static GlmTrialsPanel glm_trials_panel_of(int nj, std::integer_sequence<int, NJ...>) {
    static const GlmTrialsPanel table[] = {glm_trials_launch_panel<NJ + 1>...};
    return table[nj - 1];
}

}  // namespace chebgcn

using namespace chebgcn;

extern "C" int chebgcn_glm_trials_query(int what) {
    switch (what) {
        case 0: return GLM_VB;              // vertices of a workgroup
        case 1: return GLM_PANEL;           // trial columns of one pass over the scan
        case 2: return GLM_TRIALS_G1;       // the largest G1 = 1 + G
        case 3: return GLM_KMAX;            // the largest k = q + G of the common sums
        case 4: return GLM_TRIALS_NMAX;     // trials of one run at most
        case 5: return GLM_RMAX;            // runs of one call
        default: return -1;
    }
}

extern "C" int chebgcn_glm_trials(const float* series, int64_t Ttot, const int64_t* run_offsets, int R, int M, const double* Z, int nmax,
                                  const int64_t* trial_offsets, const double* a, const double* yy, int k, const int32_t* q_rank,
                                  const int32_t* own, const int32_t* rank, const double* w, const double* F, int G1, int64_t N,
                                  float* beta, float* variance, float* t, chebgcn_stream stream_) {
    CG_REQUIRE(series && run_offsets && Z && trial_offsets && a && yy && q_rank && own && rank && w && F, "glm_trials: NULL argument");
    CG_REQUIRE(beta || variance || t, "glm_trials: no output");
    CG_REQUIRE(Ttot >= 1 && R >= 1 && M >= 1 && M <= INT_MAX - 31 && nmax >= 1 && k >= 1 && G1 >= 1 && N >= 1,
               "glm_trials: bad shape (Ttot = %lld, R = %d, M = %d, nmax = %d, k = %d, G1 = %d, N = %lld)", (long long)Ttot, R, M, nmax, k,
               G1, (long long)N);
    const int Mp = plane_stride(M);
    if (G1 > GLM_TRIALS_G1 || k > GLM_KMAX || nmax > GLM_TRIALS_NMAX || R > GLM_RMAX || Ttot > GLM_ELEMS / Mp || N > GLM_ELEMS / Mp)
        return fail(CHEBGCN_EUNSUPPORTED,
                    "glm_trials: G1 = %d, k = %d, nmax = %d, R = %d, Ttot = %lld, N = %lld; served: G1 <= %d, k <= %d, nmax <= %d, R <= %d, "
                    "Ttot * Mp and N * Mp <= 2^39",
                    G1, k, nmax, R, (long long)Ttot, (long long)N, GLM_TRIALS_G1, GLM_KMAX, GLM_TRIALS_NMAX, GLM_RMAX);
    CG_REQUIRE(k >= G1 - 1, "glm_trials: the common sums hold k = %d planes, fewer than the G = %d sums of the other trials", k, G1 - 1);
    CG_REQUIRE((((uintptr_t)series | (uintptr_t)run_offsets | (uintptr_t)Z | (uintptr_t)trial_offsets | (uintptr_t)a | (uintptr_t)yy |
                 (uintptr_t)w | (uintptr_t)F | (uintptr_t)beta | (uintptr_t)variance | (uintptr_t)t) & 7) == 0 &&
                   (((uintptr_t)q_rank | (uintptr_t)own | (uintptr_t)rank) & 3) == 0,
               "glm_trials: unaligned argument (8 bytes, series and outputs included: a lane takes two vertices at once)");
    const GlmTrials p{series, (long long)Ttot, (const long long*)run_offsets, Z, (const long long*)trial_offsets, a, yy, q_rank, own, rank,
                      w, F, beta, variance, t, (long long)N, M, Mp, nmax, k, G1};
    const int together = CG_GLM_TRIALS_Z ? nmax / GLM_PANEL : 1;        // (nmax <= 4096: grid.z stays far below its limit)
    for (int j0 = 0; j0 < nmax;) {
        const int nj = nmax - j0 < GLM_PANEL ? nmax - j0 : GLM_PANEL;
        const int nz = j0 == 0 && together > 1 ? together : 1;
        glm_trials_panel_of(nj, std::make_integer_sequence<int, GLM_PANEL>())(j0 > 0, p, R, j0, nz, (hipStream_t)stream_);
        j0 += nj * nz;
    }
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}
