// The stages that every per-ball covariance kernel shares (searchlight_lda.hip, searchlight_rdm.hip): one workgroup of LDA_T = 256
// threads owns a row of P <= PB vertices, PB in {32, 64, 128}, and keeps in LDS the packed lower triangle of its covariance
// (element (i >= j) at i (i + 1) / 2 + j), a table of class means [PB][NCB] and a tile of LDA_TS samples' residuals
// [LDA_TS][PB + 2].  Stated once here, in the order and with the chains include/chebgcn.h states:
//   ball_covariance   the residuals of the class lists ci0 / ci1 about the table, tile by tile, added to the register-blocked
//                     chains a (thread t < 136 owns block (bi >= bj) of TB x TB elements, TB = PB / 16) and, with 'auto', to beta_;
//   ball_store        S_ij = a_ij / n into the triangle, beta_ into scal[0];
//   ball_shrinkage    trace, delta_, nu and the shrinkage g (given, or Ledoit-Wolf's): scal[1] = g, scal[2] = nu, *degen;
//   ball_sigma        Sigma = (1 - g) S + g nu I in place;
//   ball_cholesky     Sigma = L L^T in place, column by column, no pivoting;
//   ball_forward      L y = d for every column of the table at once.
// Every function is called by all threads of the workgroup; what each expects to be visible, and where it leaves a barrier, is
// said at the function.  Nothing read from memory is an address or a trip count unchecked: the callers clamp the lists.
#pragma once
#include <float.h>
#include <math.h>

#include "searchlight_common.h"

namespace chebgcn {

constexpr int LDA_T = 256;                  // threads of a workgroup
constexpr int LDA_PMAX = 128;               // the longest row
constexpr int LDA_TS = 32;                  // training samples of a residual tile
constexpr int LDA_NB = 16;                  // blocks along a side of the triangle
constexpr int LDA_BLOCKS = LDA_NB * (LDA_NB + 1) / 2;       // 136 covariance threads: waves 0 .. 2
constexpr int LDA_QW = 3;                   // the wave of the squared norms
constexpr int LDA_NARROW = 8;               // class tables in LDS are this wide up to this many classes, SL_CMAX beyond
constexpr double LDA_SHRINK_MIN = CHEBGCN_LDA_SHRINK_MIN;

static inline int lda_bucket(int P) { return P < 1 || P > LDA_PMAX ? -1 : P <= 32 ? 32 : P <= 64 ? 64 : 128; }

// The block (bi >= bj) of the triangle that thread tid owns: blocks are numbered row by row.
__device__ __forceinline__ void ball_block(int tid, int& bi, int& bj) {
    bi = 0;
    while ((bi + 1) * (bi + 2) / 2 <= tid) ++bi;
    bj = tid - bi * (bi + 1) / 2;
}

// The residual tiles of the C class lists [ci0[c], ci1[c]) of cidx, class by class, LDA_TS entries at a time in list order:
// thread (vertex, entry) reads Xt coalesced over the entries and stores r = (double)x - dw[v][c] (an entry outside [0, S): a row
// of zeros; a vertex vsh[i] < 0: a column of zeros); the loads of the next tile are issued before the arithmetic of the current
// one.  cov threads run one chain per element: a_ij = fma(r_ki, r_kj, a_ij), k in list order.  With autog the fourth wave adds
// q_k^2 to beta_, q_k = (sum of r_ki^2 over even i, ascending) + (the same over odd i).  Expects vsh, ci0, ci1 and dw visible;
// every tile ends in a barrier (no tile: no barrier).
template <int PB, int NCB>
__device__ __forceinline__ void ball_covariance(const float* Xt, int Sp, int S, const int32_t* cidx, int C, int P, const int* vsh,
                                                const int* ci0, const int* ci1, const double* dw, double* tile, int tid, int bi, int bj,
                                                bool cov, bool autog, double (&a)[PB / LDA_NB][PB / LDA_NB], double& beta_) {
    constexpr int TB = PB / LDA_NB;
    constexpr int LD = PB + 2;                                  // residual rows stay 16-byte aligned
    constexpr int NI = PB / (LDA_T / LDA_TS);                   // vertices a thread stages per tile
    static_assert(LDA_T % LDA_TS == 0 && LDA_BLOCKS <= 64 * LDA_QW && PB <= LDA_T, "thread maps");
    const int lane = tid & 63;
    const int sk = tid % LDA_TS, si = tid / LDA_TS;             // its tile entry, its first vertex
    float xr[NI];
    unsigned live = 0;                                          // bit q: xr[q] is a value
    auto next = [&](int& c, int& t) {                           // the tile after (c, t); c = C: none
        if (c >= 0 && t + LDA_TS < ci1[c]) {
            t += LDA_TS;
            return;
        }
        do ++c; while (c < C && ci0[c] >= ci1[c]);
        t = c < C ? ci0[c] : 0;
    };
    auto fetch = [&](int c, int t) {
        int j = t + sk < ci1[c] ? cidx[t + sk] : -1;
        if ((unsigned)j >= (unsigned)S) j = -1;
        live = 0;
#pragma unroll
        for (int q = 0; q < NI; ++q) {
            const int i = si + q * (LDA_T / LDA_TS);
            const int v = i < P ? vsh[i] : -1;
            xr[q] = 0.0f;
            if (j >= 0 && v >= 0) {
                xr[q] = Xt[(size_t)v * Sp + j];
                live |= 1u << q;
            }
        }
    };
    int c = -1, t0 = 0;
    next(c, t0);
    if (c < C) fetch(c, t0);
    while (c < C) {
#pragma unroll
        for (int q = 0; q < NI; ++q) {
            const int i = si + q * (LDA_T / LDA_TS);
            if (i < P) tile[sk * LD + i] = live >> q & 1 ? (double)xr[q] - dw[i * NCB + c] : 0.0;
        }
        const int kn = min(LDA_TS, ci1[c] - t0);
        next(c, t0);
        __syncthreads();
        if (c < C) fetch(c, t0);
        if (cov) {
            for (int k = 0; k < kn; ++k) {
                double ri[TB], rj[TB];
#pragma unroll
                for (int x = 0; x < TB; ++x) ri[x] = tile[k * LD + bi * TB + x];
#pragma unroll
                for (int x = 0; x < TB; ++x) rj[x] = tile[k * LD + bj * TB + x];
#pragma unroll
                for (int x = 0; x < TB; ++x)
#pragma unroll
                    for (int y = 0; y < TB; ++y) a[x][y] = fma(ri[x], rj[y], a[x][y]);
            }
        } else if (autog && tid >= 64 * LDA_QW) {
            // lanes 2 k and 2 k + 1: the even and the odd vertices of entry k
            const int k = lane >> 1, h = lane & 1;
            double part = 0.0;
            if (k < kn)
                for (int i = h; i < P; i += 2) part = fma(tile[k * LD + i], tile[k * LD + i], part);
            const double other = __shfl_xor(part, 1);
            const double q = h ? other + part : part + other;
            for (int kk = 0; kk < kn; ++kk) {
                const double qk = __shfl(q, 2 * kk);
                beta_ = fma(qk, qk, beta_);
            }
        }
        __syncthreads();
    }
}

// S_ij = a_ij / n (0 where n = 0) into the triangle, beta_ of the fourth wave into scal[0]; ends in a barrier.
template <int PB>
__device__ __forceinline__ void ball_store(double* Ssh, double* scal, int P, int n, int tid, int bi, int bj, bool cov,
                                           const double (&a)[PB / LDA_NB][PB / LDA_NB], double beta_) {
    constexpr int TB = PB / LDA_NB;
    if (cov) {
#pragma unroll
        for (int x = 0; x < TB; ++x)
#pragma unroll
            for (int y = 0; y < TB; ++y) {
                const int i = bi * TB + x, jj = bj * TB + y;
                if (i < P && jj <= i) Ssh[i * (i + 1) / 2 + jj] = n ? a[x][y] / (double)n : 0.0;
            }
    }
    if (tid == 64 * LDA_QW) scal[0] = beta_;
    __syncthreads();
}

// rowsq_i = fma chain of S_ij^2 over j < i;  thread 0:  tr = sum S_ii,  delta_ = fma(S_ii, S_ii, .), fma(2, rowsq_i, .) per i
// ascending,  nu = tr / P,  the shrinkage g (shrink, or Ledoit-Wolf's where shrink < 0: include/chebgcn.h).  Leaves scal[1] = g,
// scal[2] = nu, *degen = 1 where tr is not > 0 or n = 0 (the caller zeroed it); ends in a barrier and returns g.
__device__ __forceinline__ double ball_shrinkage(const double* Ssh, double* rowsq, double* scal, int* degen, int P, int n, double shrink,
                                                 int tid) {
    if (tid < P) {
        double s = 0.0;
        for (int jj = 0; jj < tid; ++jj) {
            const double e = Ssh[tid * (tid + 1) / 2 + jj];
            s = fma(e, e, s);
        }
        rowsq[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double tr = 0.0, dl = 0.0;
        for (int i = 0; i < P; ++i) {
            const double e = Ssh[i * (i + 1) / 2 + i];
            tr = tr + e;
            dl = fma(e, e, dl);
            dl = fma(2.0, rowsq[i], dl);
        }
        const double nu = tr / (double)P;
        double g = shrink;
        if (shrink < 0.0) {
            double beta = 0.0;
            const double delta = (dl - 2.0 * nu * tr + (double)P * nu * nu) / (double)P;
            if (n) beta = (scal[0] / (double)n - dl) / ((double)P * (double)n);
            beta = fmin(beta, delta);
            g = beta == 0.0 ? 0.0 : beta / delta;
            g = g >= LDA_SHRINK_MIN ? (g <= 1.0 ? g : 1.0) : LDA_SHRINK_MIN;        // (a NaN cannot arise: delta = 0 forces beta <= 0)
        }
        scal[1] = g;
        scal[2] = nu;
        if (!(tr > 0.0) || n == 0) *degen = 1;
    }
    __syncthreads();
    return scal[1];
}

// Sigma = (1 - g) S, g nu added to the diagonal, in place; a barrier between the two and one at the end.
__device__ __forceinline__ void ball_sigma(double* Ssh, int P, double g, double nu, int tid) {
    for (int e = tid; e < P * (P + 1) / 2; e += LDA_T) Ssh[e] = (1.0 - g) * Ssh[e];
    __syncthreads();
    if (tid < P) Ssh[tid * (tid + 1) / 2 + tid] = Ssh[tid * (tid + 1) / 2 + tid] + g * nu;
    __syncthreads();
}

// Cholesky in place, column by column: element (i, j) receives fma(-L_ik, L_jk, .) for k ascending, then sqrt (i = j) or the
// division by L_jj.  A pivot not > 0 and finite: *degen = 1 and the pivot is taken as 1 (the factor is then not used).  Every
// column ends in a barrier.
__device__ __forceinline__ void ball_cholesky(double* Ssh, int* degen, int P, int tid) {
    for (int jc = 0; jc < P; ++jc) {
        double s = 0.0;
        if (tid >= jc && tid < P) {
            const double* li = Ssh + tid * (tid + 1) / 2;
            const double* lj = Ssh + jc * (jc + 1) / 2;
            s = li[jc];
            int k = 0;
            for (; k + 4 <= jc; k += 4) {                       // (the loads of four steps before their chain)
                const double a0 = li[k], a1 = li[k + 1], a2 = li[k + 2], a3 = li[k + 3];
                const double b0 = lj[k], b1 = lj[k + 1], b2 = lj[k + 2], b3 = lj[k + 3];
                s = fma(-a0, b0, s);
                s = fma(-a1, b1, s);
                s = fma(-a2, b2, s);
                s = fma(-a3, b3, s);
            }
            for (; k < jc; ++k) s = fma(-li[k], lj[k], s);
            if (tid == jc) {
                if (!(s > 0.0) || !(s <= DBL_MAX)) {
                    *degen = 1;
                    s = 1.0;
                }
                Ssh[jc * (jc + 1) / 2 + jc] = sqrt(s);
            }
        }
        __syncthreads();
        if (tid > jc && tid < P) Ssh[tid * (tid + 1) / 2 + jc] = s / Ssh[jc * (jc + 1) / 2 + jc];
        __syncthreads();
    }
}

// L y = d for the NCB columns of dw [P][NCB] at once, thread (vertex i, class c): y_i receives fma(-L_ik, y_k, .) for k ascending,
// followed by the division by L_ii.  Expects dw visible; ends in a barrier.
template <int NCB>
__device__ __forceinline__ void ball_forward(const double* Ssh, double* dw, int P, int tid) {
    if (tid < NCB) dw[tid] = dw[tid] / Ssh[0];
    __syncthreads();
    for (int k = 0; k + 1 < P; ++k) {
        for (int e = tid; e < (P - 1 - k) * NCB; e += LDA_T) {
            const int i = k + 1 + e / NCB, c = e % NCB;
            double s = fma(-Ssh[i * (i + 1) / 2 + k], dw[k * NCB + c], dw[i * NCB + c]);
            if (i == k + 1) s = s / Ssh[i * (i + 1) / 2 + i];
            dw[i * NCB + c] = s;
        }
        __syncthreads();
    }
}

}  // namespace chebgcn
