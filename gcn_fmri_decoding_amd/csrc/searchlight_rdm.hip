// RSA searchlight (searchlight.crossnobis): the cross-validated Mahalanobis ("crossnobis") distance of every pair of classes at
// every (group, centre).  As with shrinkage LDA every pair needs its own P x P noise covariance and factor, so ONE WORKGROUP (256
// threads) owns one (centre, group) pair from the cell means -- chebgcn_searchlight_fit's par, one "model" per cell = (group,
// partition), called with eps = 0 -- to the distances, and everything in between stays in LDS.  The model: include/chebgcn.h.
//
// searchlight_rdm_kernel<PB, NCB>: PB in {32, 64, 128} the ball bucket, NCB in {8, 32} the width of the class tables in LDS.
// LDS map: the packed triangle of S / Sigma / L (PB (PB + 1) / 2 float64), the class table dw [PB][NCB] (a cell's means, later
// its d_k and u_k), the residual tile [32][PB + 2] -- free once the covariance is done, and then the home of T [PB][NCB] = sum_k
// u_k: a second table beside the tile would not fit at <128, 32> --, m, rowsq and a few rows of scalars.
//
//   1. The row (clamped; P < 1 or P > PB: the workgroup returns and touches nothing), the group's cells [k0, k1) (clamped into
//      [0, NM]; fewer than 2: the workgroup returns).
//   2. Per cell k ascending: its class lists (clamped), its counts n_kc (entries inside [0, S)), its means mu_kcv into dw;
//      m_v accumulates fma(n_kc, mu_kcv, .) over (k, c) ascending; then ball_covariance tiles the cell's class lists: the
//      register-blocked per-element chains run on ACROSS the cells, so one covariance serves all cells of the group.
//      S_ij = a_ij / n, m_v = acc / n.
//   3. ball_shrinkage, ball_sigma.   4. ball_cholesky.     (searchlight_ball.h: the stages of the LDA kernel, stated once)
//   5. Per cell k ascending: d_kcv = mu_kcv - m_v re-read from par into dw (P x C values: the cells' means cannot all stay on
//      chip), ball_forward: u_k = L^-1 d_k; T += u_k; pair thread p (and p + 256 where there are more than 256 pairs) continues
//      its chain q_ab = fma(u_kav - u_kbv, u_kav - u_kbv, q_ab) over v ascending.
//   6. t_ab = the same chain over T_av - T_bv; rdm[g][pair][u] = (t_ab - q_ab) / (F (F - 1) P); gamma_out[g][u] = g.
//      tr not > 0, n = 0 or a pivot not > 0 and finite: every distance 0 and gamma_out = -1 -- nothing is NaN.
// Every value is a function of (group, centre, the lists) alone: no float atomics, no order that depends on the launch.
// Compiler report (VGPRs, its occupancy in waves per SIMD = workgroups per CU, LDS bytes; no scratch anywhere): DESIGN 4.25.
// Nothing read from memory is an address or a trip count unchecked: row, cell and list pointers are clamped, centre numbers
// outside [0, U) end the workgroup, sample numbers outside [0, S) are rows of zeros, a vertex outside [0, M) is a column of zeros.
#include "searchlight_common.h"
#include "searchlight_ball.h"

namespace chebgcn {

constexpr int RDM_PAIRS = SL_CMAX * (SL_CMAX - 1) / 2;        // 496: at most two pairs per thread
static_assert(RDM_PAIRS <= 2 * LDA_T, "two pairs per thread");

struct SlRdm {
    const float* Xt;            // [M][Sp]
    const int32_t* rowptr;      // [U + 1]
    const int32_t* colidx;      // [nnz]
    const int32_t* centres;     // [Ub] rows of this launch
    const int32_t* cell_ptr;    // [G + 1]
    const int32_t* cptr;        // [NM * C + 1]
    const int32_t* cidx;        // [nidx]
    const double* par;          // [NM][M][NC][2]: the means at [..][c][0]
    double* rdm;                // [G][npairs][U]
    double* gamma;              // [G][U] or NULL
    double shrink;              // < 0: Ledoit-Wolf
    int S, Sp, M, nnz, U, nidx, NM, C, NC, G;
};

// block (centre blockIdx.x of the launch, group blockIdx.y)
template <int PB, int NCB>
__global__ void __launch_bounds__(LDA_T)
searchlight_rdm_kernel(SlRdm p) {
    constexpr int TB = PB / LDA_NB;
    constexpr int LD = PB + 2;
    static_assert(LDA_TS * LD >= PB * NCB, "the residual tile holds T");
    __shared__ double Ssh[PB * (PB + 1) / 2];                   // S, Sigma, L
    __shared__ double dw[PB * NCB];                             // [v][c]: mu_k, later d_k, then u_k
    __shared__ double tile[LDA_TS * LD];                        // [k][v] residuals; afterwards T [v][c]
    __shared__ double msh[PB];
    __shared__ double rowsq[PB];
    __shared__ double scal[4];                                  // beta_, g, nu
    __shared__ int vsh[PB];
    __shared__ int ncnt[NCB];
    __shared__ int ci0[NCB], ci1[NCB];                          // the class lists of the cell, clamped
    __shared__ int degen;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int grp = blockIdx.y;
    const int u = p.centres[blockIdx.x];
    if ((unsigned)u >= (unsigned)p.U) return;
    const int r0 = sl_clamp(p.rowptr[u], 0, p.nnz), r1 = sl_clamp(p.rowptr[u + 1], r0, p.nnz);
    const int P = r1 - r0;
    if (P < 1 || P > PB) return;
    const int k0 = sl_clamp(p.cell_ptr[grp], 0, p.NM), k1 = sl_clamp(p.cell_ptr[grp + 1], k0, p.NM);
    const int F = k1 - k0;
    if (F < 2) return;
    const int C = p.C;                                          // 2 <= C <= NCB: the entry point's check

    // ---- 1. row ----
    if (tid < PB) {
        const int v = tid < P ? p.colidx[r0 + tid] : -1;
        vsh[tid] = (unsigned)v < (unsigned)p.M ? v : -1;
    }
    if (tid == 0) degen = 0;

    // ---- 2. covariance about the cell means, across the cells ----
    int bi, bj;
    ball_block(tid, bi, bj);
    const bool cov = tid < LDA_BLOCKS && bi * TB < P;
    const bool autog = p.shrink < 0.0;
    double a[TB][TB];
#pragma unroll
    for (int x = 0; x < TB; ++x)
#pragma unroll
        for (int y = 0; y < TB; ++y) a[x][y] = 0.0;
    double beta_ = 0.0, macc = 0.0;
    int n = 0;
    for (int k = k0; k < k1; ++k) {
        if (tid < NCB) {
            ncnt[tid] = 0;
            const int i0 = tid < C ? sl_clamp(p.cptr[k * C + tid], 0, p.nidx) : 0;
            ci0[tid] = i0;
            ci1[tid] = tid < C ? sl_clamp(p.cptr[k * C + tid + 1], i0, p.nidx) : 0;
        }
        __syncthreads();
        for (int c = tid >> 6; c < C; c += LDA_T / 64) {        // a wave a class
            int mine = 0;
            for (int i = ci0[c] + lane; i < ci1[c]; i += 64) mine += (unsigned)p.cidx[i] < (unsigned)p.S;
            if (mine) atomicAdd(&ncnt[c], mine);
        }
        for (int e = tid; e < P * NCB; e += LDA_T) {
            const int i = e / NCB, c = e % NCB, v = vsh[i];
            dw[e] = v >= 0 && c < C ? p.par[(((size_t)k * p.M + v) * p.NC + c) * 2] : 0.0;
        }
        __syncthreads();
        for (int c = 0; c < C; ++c) n += ncnt[c];
        if (tid < P)
            for (int c = 0; c < C; ++c) macc = fma((double)ncnt[c], dw[tid * NCB + c], macc);
        ball_covariance<PB, NCB>(p.Xt, p.Sp, p.S, p.cidx, C, P, vsh, ci0, ci1, dw, tile, tid, bi, bj, cov, autog, a, beta_);
        __syncthreads();                                        // (a cell without a tile has no barrier of its own)
    }
    if (tid < P) msh[tid] = n ? macc / (double)n : 0.0;
    ball_store<PB>(Ssh, scal, P, n, tid, bi, bj, cov, a, beta_);

    // ---- 3. trace, shrinkage, Sigma ----
    const double g = ball_shrinkage(Ssh, rowsq, scal, &degen, P, n, p.shrink, tid);
    const double nu = scal[2];
    const bool flat = degen != 0;                               // uniform: nothing to factorise
    const int npairs = C * (C - 1) / 2;
    // the pairs of this thread, row-major over a < b: pair tid and pair tid + LDA_T
    int pa[2], pb[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        int rem = tid + h * LDA_T, ca = 0;
        while (ca < C - 1 && rem >= C - 1 - ca) {
            rem -= C - 1 - ca;
            ++ca;
        }
        pa[h] = ca;
        pb[h] = ca + 1 + rem;                                   // (>= C where the thread has no such pair: never used)
    }
    double q[2] = {0.0, 0.0};
    if (!flat) {
        ball_sigma(Ssh, P, g, nu, tid);
        // ---- 4. Cholesky ----
        ball_cholesky(Ssh, &degen, P, tid);
    }
    if (!flat && !degen) {                                      // (uniform: degen was last written before a barrier)
        // ---- 5. the cells: whiten, add up ----
        for (int e = tid; e < P * NCB; e += LDA_T) tile[e] = 0.0;
        for (int k = k0; k < k1; ++k) {
            for (int e = tid; e < P * NCB; e += LDA_T) {
                const int i = e / NCB, c = e % NCB, v = vsh[i];
                dw[e] = v >= 0 && c < C ? p.par[(((size_t)k * p.M + v) * p.NC + c) * 2] - msh[i] : 0.0;
            }
            __syncthreads();
            ball_forward<NCB>(Ssh, dw, P, tid);
            for (int e = tid; e < P * NCB; e += LDA_T) tile[e] = tile[e] + dw[e];
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (tid + h * LDA_T < npairs)
                    for (int i = 0; i < P; ++i) {
                        const double d = dw[i * NCB + pa[h]] - dw[i * NCB + pb[h]];
                        q[h] = fma(d, d, q[h]);
                    }
            __syncthreads();
        }
    }
    // ---- 6. the distances ----
    const bool zero = flat || degen != 0;
    const double scale = (double)F * (double)(F - 1) * (double)P;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int pair = tid + h * LDA_T;
        if (pair < npairs) {
            double t = 0.0;
            if (!zero)
                for (int i = 0; i < P; ++i) {
                    const double d = tile[i * NCB + pa[h]] - tile[i * NCB + pb[h]];
                    t = fma(d, d, t);
                }
            p.rdm[((size_t)grp * npairs + pair) * p.U + u] = zero ? 0.0 : (t - q[h]) / scale;
        }
    }
    if (tid == 0 && p.gamma) p.gamma[(size_t)grp * p.U + u] = zero ? -1.0 : g;
}

template <int PB>
static void rdm_launch(const SlRdm& p, int Ub, hipStream_t stream) {
    static char name[40];
    static const int named = snprintf(name, sizeof name, "searchlight_rdm_kernel<%d>", PB);
    (void)named;
    note_dispatch(name);
    const dim3 grid((unsigned)Ub, (unsigned)p.G);
    if (p.C <= LDA_NARROW)
        hipLaunchKernelGGL((searchlight_rdm_kernel<PB, LDA_NARROW>), grid, dim3(LDA_T), 0, stream, p);
    else
        hipLaunchKernelGGL((searchlight_rdm_kernel<PB, SL_CMAX>), grid, dim3(LDA_T), 0, stream, p);
}

}  // namespace chebgcn

using namespace chebgcn;

extern "C" int chebgcn_searchlight_rdm_query(int what) {
    switch (what) {
        case 0: return LDA_T;               // threads of a workgroup
        case 1: return LDA_PMAX;            // the longest row
        case 2: return LDA_TS;              // samples of a residual tile
        case 3: return SL_CMAX;            // the largest number of classes
        case 4: return RDM_PAIRS;           // the most pairs of classes: two per thread beyond query 0
        case 5: return SL_NMAX;            // cells of one call
        case 6: return LDA_NARROW;          // up to this many classes the class tables in LDS are this wide, query 3 beyond
        default:
            if (what > 100 && what <= 100 + LDA_PMAX) return lda_bucket(what - 100);       // the ball bucket of a row of what - 100
            return -1;
    }
}

extern "C" int chebgcn_searchlight_rdm(const float* Xt, int S, int M, const int32_t* rowptr, const int32_t* colidx, int nnz, int U,
                                       const int32_t* centres, int Ub, int bucket, const int32_t* cell_ptr, const int32_t* class_ptr,
                                       const int32_t* class_idx, int nidx, int NM, int C, const double* par, double shrinkage, int G,
                                       double* rdm, double* gamma_out, chebgcn_stream stream_) {
    CG_REQUIRE(Xt && rowptr && colidx && centres && cell_ptr && class_ptr && class_idx && par && rdm, "searchlight_rdm: NULL argument");
    CG_REQUIRE(S >= 1 && M >= 1 && S <= INT_MAX - 31 && nnz >= 1 && U >= 1 && Ub >= 1 && nidx >= 1 && NM >= 1 && C >= 2 && G >= 1 &&
                   bucket >= 1,
               "searchlight_rdm: bad shape (S = %d, M = %d, nnz = %d, U = %d, Ub = %d, %d listed samples, NM = %d, C = %d, G = %d, "
               "bucket = %d)", S, M, nnz, U, Ub, nidx, NM, C, G, bucket);
    CG_REQUIRE(shrinkage < 0.0 || (shrinkage >= LDA_SHRINK_MIN && shrinkage <= 1.0),
               "searchlight_rdm: shrinkage = %g; served: [%g, 1], or negative for Ledoit-Wolf", shrinkage, LDA_SHRINK_MIN);
    if (NM > SL_NMAX || C > SL_CMAX || (bucket != 32 && bucket != 64 && bucket != 128))
        return fail(CHEBGCN_EUNSUPPORTED, "searchlight_rdm: NM = %d, C = %d, bucket = %d; served: NM <= %d, C <= %d, bucket 32, 64 or 128",
                    NM, C, bucket, SL_NMAX, SL_CMAX);
    CG_REQUIRE(NM / 2 >= G, "searchlight_rdm: %d cells for %d groups: a group with fewer than 2 cells has no distance", NM, G);
    CG_REQUIRE((((uintptr_t)Xt | (uintptr_t)rowptr | (uintptr_t)colidx | (uintptr_t)centres | (uintptr_t)cell_ptr | (uintptr_t)class_ptr |
                 (uintptr_t)class_idx) & 3) == 0 && (((uintptr_t)par | (uintptr_t)rdm | (uintptr_t)gamma_out) & 7) == 0,
               "searchlight_rdm: unaligned argument");
    const SlRdm p{Xt, rowptr, colidx, centres, cell_ptr, class_ptr, class_idx, par, rdm, gamma_out, shrinkage, S, plane_stride(S), M, nnz, U,
                  nidx, NM, C, chebgcn_searchlight_query(100 + C), G};
    hipStream_t stream = (hipStream_t)stream_;
    switch (bucket) {
        case 32: rdm_launch<32>(p, Ub, stream); break;
        case 64: rdm_launch<64>(p, Ub, stream); break;
        default: rdm_launch<128>(p, Ub, stream); break;
    }
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}
