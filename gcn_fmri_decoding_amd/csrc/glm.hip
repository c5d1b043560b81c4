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
//   glm_project<NJ>  (its time loop is glm_pass.h, which glm_trials.hip shares)
//                    workgroup (run, 128 vertices), 4 waves: a lane owns TWO consecutive vertices (one 8-byte load per row) and
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
// AR(1) prewhitening (first_level(noise='ar1'); the algebra and the floor of its rss: include/chebgcn.h):
//   glm_project<NJ, AR1>   the same body over the table [Q | Qs] of 2k columns; the first panel also sums y_t y_{t-1}.
//   glm_finish_ar1<KB>     KB lanes per (run, vertex), KB the rank bucket: rho, the k x k system M(rho) from D and E, its
//                          Cholesky factor packed in LDS, the triangular solves for g and the contrasts; no scratch.
// No float atomics anywhere.  Nothing read from memory is an address or a trip count unchecked: run offsets are clamped into
// [0, Ttot], ranks into [0, k], run numbers of a group are skipped when outside [0, R).
#include <limits.h>

#include <utility>

#include "common.h"
#include "glm_pass.h"

namespace chebgcn {

constexpr int GLM_CMAX = 32;                // contrasts
constexpr int GLM_PMAX = 64;                // columns of a design (rows of B)
constexpr int GLM_T = 256;                  // threads of finish / combine
constexpr int GLM_SMAX = 65535;             // groups of one call (grid.z)
constexpr int GLM_AR1_NW = 4;               // waves of an AR(1) finish workgroup
constexpr int GLM_AR1_NR = 4;               // contrasts of one forward solve
constexpr double GLM_RHO_MAX = 0.99;        // an estimated coefficient is clamped to +- this

// block (GLM_VB vertices, run blockIdx.y), 4 waves; columns [j0, j0 + NJ) of Q, j0 + NJ <= k: the pass of glm_pass.h.  AR1: Q is
// the table [Q | Qs] of k columns in all, and the first panel also forms lag1[r][m] = sum_{t > t0} y_t y_{t-1}
template <int V, int NJ, bool AR1>
__global__ void __launch_bounds__(GLM_NW * 64)
glm_project_kernel(const float* __restrict__ series, long long Ttot, const long long* __restrict__ offs, int M, int Mp,
                   const double* __restrict__ Q, int k, int j0, double* __restrict__ a, double* __restrict__ yy,
                   double* __restrict__ lag1) {
    __shared__ double red[glm_pass_lds<V, NJ, AR1>()];
    const int r = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m0 = blockIdx.x * (64 * V) + lane * V;        // (Mp is a multiple of 32: a vector is inside the row or beyond it)
    const bool first = j0 == 0;
    long long t0, t1;
    glm_run(offs, r, Ttot, t0, t1);

    double acc[V][NJ], q2[V], lag[V];
    if (first) glm_pass<V, NJ, AR1, true>(acc, q2, lag, series, t0, t1, m0, M, Mp, Q, k, j0, w, lane, red);
    else glm_pass<V, NJ, AR1, false>(acc, q2, lag, series, t0, t1, m0, M, Mp, Q, k, j0, w, lane, red);
    if (w != 0 || m0 >= Mp) return;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int v = 0; v < V; ++v) a[((size_t)r * k + j0 + j) * Mp + m0 + v] = acc[v][j];
    if (first) {
#pragma unroll
        for (int v = 0; v < V; ++v) yy[(size_t)r * Mp + m0 + v] = q2[v];
        if constexpr (AR1) {
#pragma unroll
            for (int v = 0; v < V; ++v) lag1[(size_t)r * Mp + m0 + v] = lag[v];
        }
    }
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

struct GlmFinishAr1 {
    const double* ah;           // [R][2k][Mp]: a = Q^T y, then h = Qs^T y
    const double* s0;           // [R][Mp]  y.y
    const double* s1;           // [R][Mp]  sum y_t y_{t-1}
    const float* series;        // [Ttot][Mp]
    const double* W;            // [Ttot][2k] = [Q | Qs]
    const long long* offs;      // [R + 1]
    long long Ttot;
    const int32_t* rank;        // [R]
    const double* D;            // [R][k][k]
    const double* E;            // [R][k][k]
    const double* U;            // [R][C][k]
    const double* B;            // [R][P][k] or NULL
    double* eff64;              // [R][C][Mp] or NULL
    double* var64;
    float* effect;              // [R][C][Mp] or NULL
    float* variance;
    float* t;
    float* beta;                // [R][P][Mp] or NULL
    float* rho_out;             // [R][Mp]
    double rho;                 // the coefficient of every vertex when given
    int given;
    int M, Mp, k, C, P;
};

// x of row j of the lane's vertex (lane base + j).  A vertex that fills the wave takes it through a scalar register: j is the
// same in every lane
template <int KB>
__device__ __forceinline__ double glm_bcast(double x, int j, int base) {
    if constexpr (KB == 64) {
        const int lo = __builtin_amdgcn_readlane(__double2loint(x), j), hi = __builtin_amdgcn_readlane(__double2hiint(x), j);
        return __hiloint2double(hi, lo);
    } else {
        return __shfl(x, base + j, 64);
    }
}

// AR(1) generalised least squares per (run, vertex).  A rank bucket KB (8, 16, 32, 64 >= k) gives every vertex KB lanes, lane i
// = row i of the k_r x k_r system, so a wave holds 64 / KB vertices and a workgroup of 4 waves 256 / KB.  The Cholesky factor L
// of M(rho) is built column by column (left-looking): lane i forms L[i][j] = (M[i][j] - sum_{p<j} L[i][p] L[j][p]) / L[j][j],
// one fma chain over ascending p, reading its OWN row from LDS and taking L[j][p] from lane j by a cross-lane move -- every
// LDS word a lane USES it wrote itself, so the factorisation and the forward solves need no barrier; four terms of a chain
// have their reads and moves in flight together, the fmas follow in order.  LDS holds the packed
// columns, column p = rows p .. KB - 1 of every vertex of the wave, consecutive lanes on consecutive words (no bank conflict):
// 64 / KB * KB (KB + 1) / 2 doubles per wave.  M(rho) is never stored: entry (i, j) is formed from D and E (read coalesced by
// symmetry, row j across the lanes) when column j starts.  The forward solves L z = g and L w_c = u_c run column-oriented with
// the right-hand side in a register per lane, GLM_AR1_NR contrasts at a time per read of L.  The coefficients need L^-T z, which
// reads L by columns across lanes: one barrier first.  Every chain runs over ascending (the back substitution: descending)
// indices below the run's own rank k_r, and a lane beyond k_r never enters a result: nothing depends on the bucket, on the call's k
// or on the other runs.
template <int KB>
__global__ void __launch_bounds__(GLM_AR1_NW * 64)
glm_finish_ar1_kernel(GlmFinishAr1 p) {
    constexpr int VW = 64 / KB;                 // vertices of a wave
    constexpr int TRI = KB * (KB + 1) / 2;
    __shared__ double Ls[GLM_AR1_NW][VW * TRI];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int sub = lane / KB, i = lane % KB, base = sub * KB;
    const int r = blockIdx.y, k = p.k, Mp = p.Mp;
    const long long mm = ((long long)blockIdx.x * GLM_AR1_NW + wv) * VW + sub;
    const bool live = mm < Mp;                  // (no early return: every lane serves the cross-lane moves and the barrier)
    const int m = live ? (int)mm : Mp - 1;
    double* Lw = Ls[wv];
    // word of L[row][col], row >= col, of this lane's vertex
    auto at = [&](int col, int row) { return VW * (col * KB - col * (col - 1) / 2) + sub * (KB - col) + (row - col); };

    long long t0, t1;
    glm_run(p.offs, r, p.Ttot, t0, t1);
    const long long T = t1 - t0;
    const int kr = min(max(p.rank[r], 0), k);
    const long long dof = T - kr;
    const int ic = min(i, k - 1);
    const bool row = i < kr;
    const size_t k2 = 2 * (size_t)k;

    const bool data = T > 0 && mm < p.M;        // the pad columns of the series never reach a result
    const long long ra = min(t0, p.Ttot - 1), rb = max(t1 - 1, 0LL);
    const float f0 = p.series[(size_t)ra * Mp + m], fL = p.series[(size_t)rb * Mp + m];
    const double y0 = data ? (double)f0 : 0.0, yL = data ? (double)fL : 0.0;
    const double w0 = p.W[(size_t)ra * k2 + ic], wL = p.W[(size_t)rb * k2 + ic];
    const double q0 = row && T > 0 ? w0 : 0.0, qL = row && T > 0 ? wL : 0.0;
    const double av = p.ah[((size_t)r * k2 + ic) * Mp + m], hv = p.ah[((size_t)r * k2 + k + ic) * Mp + m];
    const double a = row ? av : 0.0, h = row ? hv : 0.0;
    const double S0 = p.s0[(size_t)r * Mp + m], S1 = p.s1[(size_t)r * Mp + m];
    const double* Dr = p.D + (size_t)r * k * k + ic;
    const double* Er = p.E + (size_t)r * k * k + ic;

    double rho = p.rho;
    if (!p.given) {
        double ssq = 0.0, ahs = 0.0, da = 0.0, ada = 0.0;
        for (int j = 0; j < kr; ++j) {
            const double aj = glm_bcast<KB>(a, j, base), hj = glm_bcast<KB>(h, j, base);
            ssq = fma(aj, aj, ssq);
            ahs = fma(aj, hj, ahs);
            da = fma(Dr[(size_t)j * k], aj, da);                // (D a)_i, D symmetric
        }
        for (int j = 0; j < kr; ++j) ada = fma(glm_bcast<KB>(a, j, base), glm_bcast<KB>(da, j, base), ada);
        double rss = S0 - ssq;
        if (rss < 4.0 * (double)(T + kr) * 0x1p-53 * S0) rss = 0.0;
        const double num = (S1 - ahs) + 0.5 * ada;
        rho = rss > 0.0 ? num / rss : 0.0;
        rho = rho > GLM_RHO_MAX ? GLM_RHO_MAX : rho < -GLM_RHO_MAX ? -GLM_RHO_MAX : rho;
        if (!(rho == rho)) rho = 0.0;
    }
    const double r2 = rho * rho, c1 = fma(rho, rho, 1.0);
    const double g = fma(-r2, fma(q0, y0, qL * yL), fma(-rho, h, c1 * a));
    const double yKy = fma(-r2, fma(y0, y0, yL * yL), fma(-2.0 * rho, S1, c1 * S0));

    // M = L L^T
    double dinv = 0.0;                          // 1 / L[i][i]
    double dn = Dr[0], en = Er[0];              // row j of D and E, loaded a column ahead
    for (int j = 0; j < kr; ++j) {
        double acc = fma(-r2, en, fma(-rho, dn, i == j ? c1 : 0.0));
        const size_t nx = (size_t)min(j + 1, k - 1) * k;
        dn = Dr[nx];
        en = Er[nx];
        // L[i][q] x L[j][q], q ascending: four reads and four cross-lane moves in flight, then their fmas in order.  A lane
        // above the column (i < q) forms the same address expression, which then points below its slot but inside the wave's
        // block (column q starts at a word >= q); what it reads there is never used
        int q = 0;
        for (; q + 4 <= j; q += 4) {
            double x[4], l[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = Lw[at(q + u, i)];
#pragma unroll
            for (int u = 0; u < 4; ++u) l[u] = glm_bcast<KB>(x[u], j, base);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = fma(-x[u], l[u], acc);
        }
        for (; q < j; ++q) {
            const double x = Lw[at(q, i)];
            acc = fma(-x, glm_bcast<KB>(x, j, base), acc);
        }
        const double piv = glm_bcast<KB>(acc, j, base);
        const double d = piv > 0.0 ? sqrt(piv) : 0.0;
        const double di = d > 0.0 ? 1.0 / d : 0.0;
        if (i >= j && row) Lw[at(j, i)] = i == j ? d : acc * di;
        if (i == j) dinv = di;
    }

    // L z = g
    double z = g, zz = 0.0;
    for (int j = 0; j < kr; ++j) {
        const double l = Lw[at(j, i)];                          // (i < j: as above, unused)
        const double zj = glm_bcast<KB>(z * dinv, j, base);
        zz = fma(zj, zj, zz);
        if (i > j) z = fma(-l, zj, z);
    }
    z = row ? z * dinv : 0.0;
    const double ar = fabs(rho), up = (1.0 + ar) * (1.0 + ar), lo = (1.0 - ar) * (1.0 - ar);
    const double grow = up * up / lo;           // |M| |M^-1 g|^2 <= (1 + |rho|)^4 / (1 - |rho|)^2 y.y: the header derives it
    double rss = yKy - zz;
    if (rss < 4.0 * (double)(T + kr) * 0x1p-53 * grow * S0) rss = 0.0;
    const double s2 = dof > 0 ? rss / (double)dof : 0.0;
    if (live && i == 0) p.rho_out[(size_t)r * Mp + m] = (float)rho;

    // L w_c = u_c, GLM_AR1_NR contrasts per read of L
    for (int c0 = 0; c0 < p.C; c0 += GLM_AR1_NR) {
        double w[GLM_AR1_NR], e[GLM_AR1_NR], ww[GLM_AR1_NR];
#pragma unroll
        for (int n = 0; n < GLM_AR1_NR; ++n) {
            const double u = p.U[((size_t)r * p.C + min(c0 + n, p.C - 1)) * k + ic];
            w[n] = row && c0 + n < p.C ? u : 0.0;
            e[n] = ww[n] = 0.0;
        }
        for (int j = 0; j < kr; ++j) {
            const double l = Lw[at(j, i)];
            const double zj = glm_bcast<KB>(z, j, base);
#pragma unroll
            for (int n = 0; n < GLM_AR1_NR; ++n) {
                const double wj = glm_bcast<KB>(w[n] * dinv, j, base);
                ww[n] = fma(wj, wj, ww[n]);
                e[n] = fma(wj, zj, e[n]);
                if (i > j) w[n] = fma(-l, wj, w[n]);
            }
        }
        if (live && i == 0) {
#pragma unroll
            for (int n = 0; n < GLM_AR1_NR; ++n) {
                if (c0 + n >= p.C) break;
                const double v = s2 * ww[n];
                const double tv = v > 0.0 ? e[n] / sqrt(v) : 0.0;
                const size_t o = ((size_t)r * p.C + c0 + n) * Mp + m;
                if (p.eff64) p.eff64[o] = e[n];
                if (p.var64) p.var64[o] = v;
                if (p.effect) p.effect[o] = (float)e[n];
                if (p.variance) p.variance[o] = (float)v;
                if (p.t) p.t[o] = (float)tv;
            }
        }
    }

    if (!p.beta) return;                        // (the same in every thread)
    __syncthreads();                            // from here a lane reads words of L that other lanes wrote
    // L^T v = z, rows descending: lane i collects - L[q][i] v_q for q > i
    double v = z;
    for (int q = kr - 1; q >= 0; --q) {
        const double l = Lw[at(min(i, q), q)];
        const double vq = glm_bcast<KB>(v * dinv, q, base);
        if (i < q) v = fma(-l, vq, v);
    }
    v = row ? v * dinv : 0.0;
    for (int pc = 0; pc < p.P; pc += KB) {      // b = B v, lane i the coefficient pc + i
        const int pp = pc + i;
        const double* b = p.B + ((size_t)r * p.P + min(pp, p.P - 1)) * k;
        double s = 0.0;
        for (int j = 0; j < kr; ++j) s = fma(b[j], glm_bcast<KB>(v, j, base), s);
        if (live && pp < p.P) p.beta[((size_t)r * p.P + pp) * Mp + m] = (float)s;
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
template <int NJ, bool AR1>
static int glm_launch_panel(bool more, const float* series, long long Ttot, const long long* offs, int R, int M, int Mp, const double* Q,
                            int k, int j0, double* a, double* yy, double* lag1, hipStream_t stream) {
    static char name[40];
    static const int named = snprintf(name, sizeof name, AR1 ? "glm_project_ar1_kernel<%d>" : "glm_project_kernel<%d>", NJ);
    (void)named;
    if (more) note_dispatch_more(name);
    else note_dispatch(name);
    const dim3 grid((unsigned)((Mp + GLM_VB - 1) / GLM_VB), (unsigned)R);
    hipLaunchKernelGGL((glm_project_kernel<GLM_V, NJ, AR1>), grid, dim3(GLM_NW * 64), 0, stream, series, Ttot, offs, M, Mp, Q, k, j0, a,
                       yy, lag1);
    return CHEBGCN_OK;
}

typedef int (*GlmPanel)(bool, const float*, long long, const long long*, int, int, int, const double*, int, int, double*, double*,
                        double*, hipStream_t);
template <bool AR1, int... NJ>
static GlmPanel glm_panel_of(int nj, std::integer_sequence<int, NJ...>) {
    static const GlmPanel table[] = {glm_launch_panel<NJ + 1, AR1>...};
    return table[nj - 1];
}

// every panel of a table of k columns, GLM_PANEL at a time
template <bool AR1>
static void glm_project_panels(const float* series, long long Ttot, const long long* offs, int R, int M, int Mp, const double* Q, int k,
                               double* a, double* yy, double* lag1, hipStream_t stream) {
    for (int j0 = 0; j0 < k; j0 += GLM_PANEL) {
        const int nj = k - j0 < GLM_PANEL ? k - j0 : GLM_PANEL;
        glm_panel_of<AR1>(nj, std::make_integer_sequence<int, GLM_PANEL>())(j0 > 0, series, Ttot, offs, R, M, Mp, Q, k, j0, a, yy, lag1,
                                                                            stream);
    }
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
    glm_project_panels<false>(series, (long long)Ttot, (const long long*)run_offsets, R, M, Mp, Q, k, a, yy, nullptr, (hipStream_t)stream_);
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

// ---- AR(1) prewhitened fits (first_level(noise='ar1')) ----

namespace chebgcn {

static inline int glm_ar1_bucket(int k) { return k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : 64; }

template <int KB>
static void glm_launch_finish_ar1(const GlmFinishAr1& p, int R, hipStream_t stream) {
    static char name[40];
    static const int named = snprintf(name, sizeof name, "glm_finish_ar1_kernel<%d>", KB);
    (void)named;
    note_dispatch(name);
    const int per = GLM_AR1_NW * (64 / KB);
    hipLaunchKernelGGL(glm_finish_ar1_kernel<KB>, dim3((unsigned)((p.Mp + per - 1) / per), (unsigned)R), dim3(GLM_AR1_NW * 64), 0, stream, p);
}

}  // namespace chebgcn

extern "C" int chebgcn_glm_ar1_query(int what) {
    if (what == 0) return GLM_AR1_NW;                                           // waves of a finish workgroup
    if (what == 1) return GLM_AR1_NR;                                           // contrasts of one forward solve
    if (what > 100 && what <= 100 + GLM_KMAX) return glm_ar1_bucket(what - 100);                            // rank bucket of k
    if (what > 200 && what <= 200 + GLM_KMAX) return GLM_AR1_NW * (64 / glm_ar1_bucket(what - 200));        // vertices of a workgroup
    return -1;
}

extern "C" size_t chebgcn_glm_ar1_workspace(int R, int M, int k) {
    if (!glm_shape_ok(R, M) || R > GLM_RMAX || k < 1 || k > GLM_KMAX || M > INT_MAX - 31) return 0;
    return (size_t)R * (size_t)(2 * k + 2) * (size_t)plane_stride(M) * sizeof(double);
}

extern "C" int chebgcn_glm_project_ar1(const float* series, int64_t Ttot, const int64_t* run_offsets, int R, int M, const double* W, int k,
                                       double* ah, double* s0, double* s1, chebgcn_stream stream_) {
    CG_REQUIRE(series && run_offsets && W && ah && s0 && s1, "glm_project_ar1: NULL argument");
    CG_REQUIRE(Ttot >= 1 && glm_shape_ok(R, M) && k >= 1 && M <= INT_MAX - 31,
               "glm_project_ar1: bad shape (Ttot = %lld, R = %d, M = %d, k = %d)", (long long)Ttot, R, M, k);
    const int Mp = plane_stride(M);
    if (k > GLM_KMAX || R > GLM_RMAX || Ttot > GLM_ELEMS / Mp)
        return fail(CHEBGCN_EUNSUPPORTED, "glm_project_ar1: k = %d, R = %d, Ttot = %lld; served: k <= %d, R <= %d, Ttot * Mp <= 2^39", k, R,
                    (long long)Ttot, GLM_KMAX, GLM_RMAX);
    CG_REQUIRE((((uintptr_t)series | (uintptr_t)run_offsets | (uintptr_t)W | (uintptr_t)ah | (uintptr_t)s0 | (uintptr_t)s1) & 7) == 0,
               "glm_project_ar1: unaligned argument (8 bytes, series included: a lane loads two vertices at once)");
    glm_project_panels<true>(series, (long long)Ttot, (const long long*)run_offsets, R, M, Mp, W, 2 * k, ah, s0, s1, (hipStream_t)stream_);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_glm_finish_ar1(const double* ah, const double* s0, const double* s1, const float* series, const double* W,
                                      const int64_t* run_offsets, int64_t Ttot, const int32_t* rank, const double* D, const double* E,
                                      const double* U, const double* B, int R, int M, int k, int C, int P, int rho_given, double rho,
                                      double* eff64, double* var64, float* effect, float* variance, float* t, float* beta,
                                      float* rho_out, chebgcn_stream stream_) {
    CG_REQUIRE(ah && s0 && s1 && series && W && run_offsets && rank && D && E && U && rho_out, "glm_finish_ar1: NULL argument");
    CG_REQUIRE((eff64 && var64) || (effect && variance && t) || beta, "glm_finish_ar1: no output");
    CG_REQUIRE(!eff64 == !var64 && !effect == !variance && !effect == !t, "glm_finish_ar1: effect, variance (and t) come together");
    CG_REQUIRE(!beta == !B, "glm_finish_ar1: beta and B come together");
    CG_REQUIRE(Ttot >= 1 && glm_shape_ok(R, M) && k >= 1 && C >= 1 && P >= 0 && (P >= 1 || !beta) && M <= INT_MAX - 31,
               "glm_finish_ar1: bad shape (Ttot = %lld, R = %d, M = %d, k = %d, C = %d, P = %d)", (long long)Ttot, R, M, k, C, P);
    CG_REQUIRE(rho_given == 0 || rho_given == 1, "glm_finish_ar1: rho_given must be 0 or 1, got %d", rho_given);
    CG_REQUIRE(!rho_given || (rho > -1.0 && rho < 1.0), "glm_finish_ar1: a given rho must lie inside (-1, 1), got %g", rho);
    const int Mp = plane_stride(M);
    if (k > GLM_KMAX || C > GLM_CMAX || P > GLM_PMAX || R > GLM_RMAX || Ttot > GLM_ELEMS / Mp)
        return fail(CHEBGCN_EUNSUPPORTED,
                    "glm_finish_ar1: k = %d, C = %d, P = %d, R = %d, Ttot = %lld; served: k <= %d, C <= %d, P <= %d, R <= %d, Ttot * Mp <= 2^39",
                    k, C, P, R, (long long)Ttot, GLM_KMAX, GLM_CMAX, GLM_PMAX, GLM_RMAX);
    CG_REQUIRE((((uintptr_t)ah | (uintptr_t)s0 | (uintptr_t)s1 | (uintptr_t)W | (uintptr_t)run_offsets | (uintptr_t)D | (uintptr_t)E |
                 (uintptr_t)U | (uintptr_t)B | (uintptr_t)eff64 | (uintptr_t)var64) & 7) == 0 &&
                   (((uintptr_t)series | (uintptr_t)rank | (uintptr_t)effect | (uintptr_t)variance | (uintptr_t)t | (uintptr_t)beta |
                     (uintptr_t)rho_out) & 3) == 0,
               "glm_finish_ar1: unaligned argument");
    GlmFinishAr1 p{ah, s0, s1, series, W, (const long long*)run_offsets, (long long)Ttot, rank, D, E, U, B, eff64, var64, effect, variance,
                   t, beta, rho_out, rho_given ? rho : 0.0, rho_given, M, Mp, k, C, P};
    switch (glm_ar1_bucket(k)) {
        case 8: glm_launch_finish_ar1<8>(p, R, (hipStream_t)stream_); break;
        case 16: glm_launch_finish_ar1<16>(p, R, (hipStream_t)stream_); break;
        case 32: glm_launch_finish_ar1<32>(p, R, (hipStream_t)stream_); break;
        default: glm_launch_finish_ar1<64>(p, R, (hipStream_t)stream_); break;
    }
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}
