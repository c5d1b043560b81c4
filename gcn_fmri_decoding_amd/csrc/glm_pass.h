// The pass over the scan that glm.hip (the projections on a design's basis) and glm_trials.hip (the projections on a run's
// trial columns) share: a workgroup of GLM_NW waves takes (run, GLM_VB vertices) and NJ columns of a float64 table whose rows
// run with the scan's; a lane owns GLM_V consecutive vertices, GLM_U rows are in flight while the GLM_U before them are worked
// on, a table row comes through the scalar cache, and a run of T >= GLM_SPLIT rows is cut into slices that are a function of T
// ALONE, their sums added to wave 0's in ascending order through LDS.  glm.hip tells why each of these is as it is.
#pragma once

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
constexpr int GLM_SLICE = 32;               // a wave's slice is at least this many rows
constexpr int GLM_SPLIT = 2 * GLM_SLICE;    // runs from this length are split
constexpr int GLM_RMAX = 65535;             // runs of one call (grid.y)
constexpr long long GLM_ELEMS = 0x7fffffffffLL;   // Ttot * Mp at most

// rows [t0, t1) of run r inside [0, Ttot]; a descending pair is an empty run
__device__ __forceinline__ void glm_run(const long long* __restrict__ offs, int r, long long Ttot, long long& t0, long long& t1) {
    t0 = min(max(offs[r], 0LL), Ttot);
    t1 = min(max(offs[r + 1], t0), Ttot);
}

// AR1: the first panel also sums the lag products y_t y_{t-1} (lag) against the row before (prv), which it then replaces
template <int V, int NJ, bool AR1>
__device__ __forceinline__ void glm_row(double (&acc)[V][NJ], double (&q2)[V], double (&lag)[V], double (&prv)[V], const float (&y)[V],
                                        const double* __restrict__ q, bool first) {
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
        if constexpr (AR1) {
#pragma unroll
            for (int v = 0; v < V; ++v) {
                lag[v] = fma(yd[v], prv[v], lag[v]);
                prv[v] = yd[v];
            }
        }
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

// doubles of LDS the pass needs: the sums of a lane and vertex that cross the slices
template <int V, int NJ, bool AR1>
constexpr int glm_pass_lds() { return V * (NJ + (AR1 ? 2 : 1)) * 64; }

// Columns [j0, j0 + NJ) of the table Q (k columns in all, j0 + NJ <= k) against rows [t0, t1) of the scan, vertices [m0, m0 + V)
// of this lane; called by every thread of the workgroup (it holds barriers), w its wave, red its LDS.  On return wave 0 holds
// in acc (and, with YY -- the first panel of a table that wants y.y -- in q2 and lag) the sums over the whole run; what the
// other waves hold is their slice's.  YY is a template flag and not a value: with the flag inside the loop the compiler
// unswitches it and schedules the table's scalar loads of the other arm behind their waits (measured: 0.64 ms against 0.43 ms).
// AR1: the first panel also forms lag = sum_{t > t0} y_t y_{t-1}: the term of row t belongs to the slice of row t (the first row
// of a later slice pairs with the last row of the slice before it, the first row of the run with nothing: a lag never crosses
// a run boundary)
template <int V, int NJ, bool AR1, bool YY>
__device__ __forceinline__ void glm_pass(double (&acc)[V][NJ], double (&q2)[V], double (&lag)[V], const float* __restrict__ series,
                                         long long t0, long long t1, int m0, int M, int Mp, const double* __restrict__ Q, int k, int j0,
                                         int w, int lane, double* red) {
    constexpr int NS = NJ + (AR1 ? 2 : 1);
    constexpr bool first = YY;                  // whether this pass also sums y.y (and the lag products): the first panel's does
    const long long T = t1 - t0;
    const int nsl = T < GLM_SPLIT ? 1 : (int)min((long long)GLM_NW, T / GLM_SLICE);
    const long long len = (T + nsl - 1) / nsl;
    const long long ta = min(t0 + (long long)w * len, t1), tb = w < nsl ? min(ta + len, t1) : ta;

    double prv[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        q2[v] = lag[v] = prv[v] = 0.0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[v][j] = 0.0;
    }
    // GLM_U rows in flight while the GLM_U before them are worked on.  No load stands behind a branch (the compiler would wait for
    // each one at the join): a row at or beyond tb is read as row tb - 1 and never used
    if (ta < tb) {
        float cur[GLM_U][V], nxt[GLM_U][V];
        if constexpr (AR1) {                    // the row before the slice; the run's first row pairs with 0 (y * 0 adds +0)
            float y[V];
            glm_load<V>(y, series + (size_t)max(ta - 1, t0) * Mp, m0, M, Mp);
#pragma unroll
            for (int v = 0; v < V; ++v) prv[v] = ta > t0 ? (double)y[v] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < GLM_U; ++u) glm_load<V>(cur[u], series + (size_t)min(ta + u, tb - 1) * Mp, m0, M, Mp);
        for (long long t = ta; t < tb; t += GLM_U) {
#pragma unroll
            for (int u = 0; u < GLM_U; ++u) glm_load<V>(nxt[u], series + (size_t)min(t + GLM_U + u, tb - 1) * Mp, m0, M, Mp);
            if (t + GLM_U <= tb) {
#pragma unroll
                for (int u = 0; u < GLM_U; ++u) glm_row<V, NJ, AR1>(acc, q2, lag, prv, cur[u], Q + (size_t)(t + u) * k + j0, first);
            } else {
#pragma unroll
                for (int u = 0; u < GLM_U; ++u)
                    if (t + u < tb) glm_row<V, NJ, AR1>(acc, q2, lag, prv, cur[u], Q + (size_t)(t + u) * k + j0, first);
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
                for (int j = 0; j < NJ; ++j) red[(v * NS + j) * 64 + lane] = acc[v][j];
                red[(v * NS + NJ) * 64 + lane] = q2[v];
                if constexpr (AR1) red[(v * NS + NJ + 1) * 64 + lane] = lag[v];
            }
        }
        __syncthreads();
        if (w == 0) {
#pragma unroll
            for (int v = 0; v < V; ++v) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[v][j] = acc[v][j] + red[(v * NS + j) * 64 + lane];
                q2[v] = q2[v] + red[(v * NS + NJ) * 64 + lane];
                if constexpr (AR1) lag[v] = lag[v] + red[(v * NS + NJ + 1) * 64 + lane];
            }
        }
        __syncthreads();
    }
}

}  // namespace chebgcn
