// Searchlight decoding with shrinkage LDA (searchlight.searchlight(classifier='lda')): every (training set, centre) pair gets its
// own pooled within-class covariance of the ball, shrunk towards a multiple of the identity, its Cholesky factor and its
// discriminants.  No per-vertex table can serve that, so ONE WORKGROUP (256 threads) owns one (centre, model) pair from the class
// means -- chebgcn_searchlight_fit's par, called with eps = 0 -- to the counts, and everything in between stays in LDS.
//
// searchlight_lda_kernel<PB, NCB>: PB in {32, 64, 128} the ball bucket (a row of P <= PB vertices), NCB in {8, 32} the width of the
// class tables in LDS.  LDS: the packed lower triangle of S (PB (PB + 1) / 2 float64: 66 048 B at PB = 128), mu / d / w [PB][NCB]
// (32 KiB at 128 x 32), m, a tile of 32 training samples' residuals [32][PB + 2] float64 (which holds a copy of d afterwards), and
// a few rows of scalars: 134 KiB at <128, 32>, 23 KiB at <32, 8>.  All arithmetic is float64.
//
//   1. The row (clamped; P < 1 or P > PB: the workgroup returns and touches nothing), the class counts n_c (entries of the class
//      list inside [0, S)), n = sum n_c, mu_cv from par, m_v = (acc = 0; acc = fma(n_c, mu_cv, acc), c ascending) / n.
//   2. The covariance.  Per class c ascending and per tile of 32 entries of its list in list order: thread (vertex, entry) reads
//      Xt coalesced over the entries and stores r = (double)x - mu_cv (an entry outside [0, S): a row of zeros); the loads of the
//      next tile are issued before the arithmetic of the current one.  The triangle is
//      cut into 16 x 16 blocks of TB x TB elements, TB = PB / 16; thread t < 136 owns block (bi >= bj) in TB x TB registers and
//      runs ONE CHAIN OVER THE SAMPLES per element: a_ij = fma(r_ki, r_kj, a_ij), k in list order, class 0's list first.  Per
//      sample an 8 x 8 block reads 128 B of LDS for 64 FMAs, which is what LDS can feed the float64 ALU.  Blocks are numbered row
//      by row, so the waves beyond the row's P do nothing.  The fourth wave is free: with shrinkage 'auto' it forms the squared
//      norm of every residual, q_k = (sum of r_ki^2 over even i, ascending) + (the same over odd i), and
//      beta_ = fma(q_k, q_k, beta_) in list order.  S_ij = a_ij / n.
//   3. rowsq_i = fma chain of S_ij^2 over j < i;  thread 0:  tr = sum S_ii,  delta_ = fma(S_ii, S_ii, .), fma(2, rowsq_i, .) per i
//      ascending,  nu = tr / P,  the shrinkage g (given, or Ledoit-Wolf: include/chebgcn.h).  Sigma = (1 - g) S, g nu added to the
//      diagonal, in place;  d = mu - m in place, and a copy of it in the tile.
//   4. Cholesky in place, column by column: element (i, j) receives fma(-L_ik, L_jk, .) for k ascending, then sqrt (i = j) or the
//      division by L_jj.  No pivoting: g >= 1e-6 bounds the condition number by about P / g.
//   5. L y = d and L^T w = y for all classes at once, thread (vertex, class): y_i receives fma(-L_ik, y_k, .) for k ascending, w_i
//      receives fma(-L_ki, w_k, .) for k DEscending, each followed by the division by L_ii.
//      b_c = logprior_c - 0.5 (acc = 0; acc = fma(d_cv, w_cv, acc), v ascending).
//      tr not > 0, n = 0 or a pivot not > 0 and finite:  w = 0, b = logprior -- the prior decides, nothing is NaN.
//   6. The model's test samples, 256 per pass, a lane a sample: a_c = 0; t = (double)x - m_v; a_c = fma(w_cv, t, a_c), v ascending;
//      score_c = b_c + a_c; the first maximal class; the counts by sl_tally of searchlight_common.h (ballot, one int32 atomic per
//      distinct (group, label) of a wave).
// Every value is a function of (model, centre, the lists) alone: no float atomics, no order that depends on the launch.
// Compiler report (VGPRs, its occupancy in waves per SIMD = workgroups per CU, LDS bytes; no scratch anywhere): <32, 8> 108, 4,
// 15 816; <32, 32> 185, 2, 22 440; <64, 8> 92, 4, 39 112; <64, 32> 185, 2, 51 880; <128, 8> 219, 1, 110 280; <128, 32> 221, 1,
// 135 336 (the LDS admits one).  Measured, and what bounds it (the chain of stages of one workgroup): DESIGN 4.24.
// Nothing read from memory is an address or a trip count unchecked: row, list and test pointers are clamped, centre numbers
// outside [0, U) end the workgroup, sample numbers outside [0, S) are rows of zeros, a vertex outside [0, M) is a column of zeros
// (its w is 0), group and label numbers outside their ranges add nothing.
// Stages 2 to 4 and the forward solve of stage 5 are stated in searchlight_ball.h, which searchlight_rdm.hip shares.
#include "searchlight_common.h"
#include "searchlight_ball.h"

namespace chebgcn {

constexpr int LDA_SU = 16;                  // vertices of a scoring lane in flight (the loop is bound by the latency of Xt)

struct SlLda {
    const float* Xt;            // [M][Sp]
    const int32_t* rowptr;      // [U + 1]
    const int32_t* colidx;      // [nnz]
    const int32_t* centres;     // [Ub] rows of this launch
    const int32_t* cptr;        // [NM * C + 1]
    const int32_t* cidx;        // [nidx]
    const int32_t* tptr;        // [NM + 1]
    const double* par;          // [NM][M][NC][2]: the means at [..][c][0]
    const double* logprior;     // [NM][NC]
    const int32_t* sgroup;      // [S]
    const int32_t* slabel;      // [S]
    const int32_t* sorig;       // [S]
    int32_t* correct;           // [G][C][U]
    double* scores;             // [S][C][U] or NULL
    uint8_t* predictions;       // [S][U] or NULL
    double* gamma;              // [NM][U] or NULL
    double shrink;              // < 0: Ledoit-Wolf
    int S, Sp, M, nnz, U, nidx, tmax, C, NC, G;
};

// block (centre blockIdx.x of the launch, model blockIdx.y)
template <int PB, int NCB>
__global__ void __launch_bounds__(LDA_T)
searchlight_lda_kernel(SlLda p) {
    constexpr int TB = PB / LDA_NB;
    constexpr int LD = PB + 2;                                  // residual rows stay 16-byte aligned
    static_assert(LDA_TS * LD >= PB * NCB, "the residual tile holds the copy of d");
    static_assert(LDA_T % LDA_TS == 0 && LDA_BLOCKS <= 64 * LDA_QW && PB <= LDA_T, "thread maps");
    __shared__ double Ssh[PB * (PB + 1) / 2];                   // S, Sigma, L: element (i >= j) at i (i + 1) / 2 + j
    __shared__ double dw[PB * NCB];                             // [v][c]: mu, then d, then y, then w
    __shared__ double tile[LDA_TS * LD];                        // [k][v] residuals; afterwards d [v][c]
    __shared__ double msh[PB];
    __shared__ double rowsq[PB];
    __shared__ double bsh[NCB];
    __shared__ double scal[4];                                  // beta_, g, nu
    __shared__ int vsh[PB];
    __shared__ int ncnt[NCB];
    __shared__ int ci0[NCB], ci1[NCB];                          // the class lists, clamped
    __shared__ int degen;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int m = blockIdx.y;
    const int u = p.centres[blockIdx.x];
    if ((unsigned)u >= (unsigned)p.U) return;
    const int r0 = sl_clamp(p.rowptr[u], 0, p.nnz), r1 = sl_clamp(p.rowptr[u + 1], r0, p.nnz);
    const int P = r1 - r0;
    if (P < 1 || P > PB) return;
    const int C = p.C;                                          // 2 <= C <= NCB: the entry point's check

    // ---- 1. row, counts, means ----
    if (tid < PB) {
        const int v = tid < P ? p.colidx[r0 + tid] : -1;
        vsh[tid] = (unsigned)v < (unsigned)p.M ? v : -1;
    }
    if (tid < NCB) {
        ncnt[tid] = 0;
        const int i0 = tid < C ? sl_clamp(p.cptr[m * C + tid], 0, p.nidx) : 0;
        ci0[tid] = i0;
        ci1[tid] = tid < C ? sl_clamp(p.cptr[m * C + tid + 1], i0, p.nidx) : 0;
    }
    if (tid == 0) degen = 0;
    __syncthreads();
    for (int c = tid >> 6; c < C; c += LDA_T / 64) {            // a wave a class
        int mine = 0;
        for (int i = ci0[c] + lane; i < ci1[c]; i += 64) mine += (unsigned)p.cidx[i] < (unsigned)p.S;
        if (mine) atomicAdd(&ncnt[c], mine);
    }
    for (int e = tid; e < P * NCB; e += LDA_T) {
        const int i = e / NCB, c = e % NCB, v = vsh[i];
        dw[e] = v >= 0 && c < C ? p.par[(((size_t)m * p.M + v) * p.NC + c) * 2] : 0.0;
    }
    __syncthreads();
    int n = 0;
    for (int c = 0; c < C; ++c) n += ncnt[c];
    if (tid < P) {
        double acc = 0.0;
        for (int c = 0; c < C; ++c) acc = fma((double)ncnt[c], dw[tid * NCB + c], acc);
        msh[tid] = n ? acc / (double)n : 0.0;
    }

    // ---- 2. covariance ----
    int bi, bj;
    ball_block(tid, bi, bj);
    const bool cov = tid < LDA_BLOCKS && bi * TB < P;
    const bool autog = p.shrink < 0.0;
    double a[TB][TB];
#pragma unroll
    for (int x = 0; x < TB; ++x)
#pragma unroll
        for (int y = 0; y < TB; ++y) a[x][y] = 0.0;
    double beta_ = 0.0;
    ball_covariance<PB, NCB>(p.Xt, p.Sp, p.S, p.cidx, C, P, vsh, ci0, ci1, dw, tile, tid, bi, bj, cov, autog, a, beta_);
    ball_store<PB>(Ssh, scal, P, n, tid, bi, bj, cov, a, beta_);

    // ---- 3. trace, shrinkage, Sigma ----
    const double g = ball_shrinkage(Ssh, rowsq, scal, &degen, P, n, p.shrink, tid);
    const double nu = scal[2];
    if (tid == 0 && p.gamma) p.gamma[(size_t)m * p.U + u] = g;
    const bool flat = degen != 0;                               // uniform: nothing to factorise
    for (int e = tid; e < P * NCB; e += LDA_T) {
        const double d = e % NCB < C ? dw[e] - msh[e / NCB] : 0.0;
        dw[e] = d;
        tile[e] = d;
    }
    ball_sigma(Ssh, P, g, nu, tid);

    if (!flat) {
        // ---- 4. Cholesky ----
        ball_cholesky(Ssh, &degen, P, tid);
        // ---- 5. the solves: thread (vertex i, class c) ----
        ball_forward<NCB>(Ssh, dw, P, tid);
        if (tid < NCB) dw[(P - 1) * NCB + tid] = dw[(P - 1) * NCB + tid] / Ssh[(P - 1) * P / 2 + P - 1];
        __syncthreads();
        for (int k = P - 1; k > 0; --k) {
            for (int e = tid; e < k * NCB; e += LDA_T) {
                const int i = e / NCB, c = e % NCB;
                double s = fma(-Ssh[k * (k + 1) / 2 + i], dw[k * NCB + c], dw[i * NCB + c]);
                if (i == k - 1) s = s / Ssh[i * (i + 1) / 2 + i];
                dw[i * NCB + c] = s;
            }
            __syncthreads();
        }
    }
    if (degen) {                                                // (uniform: degen was last written before a barrier)
        for (int e = tid; e < P * NCB; e += LDA_T) dw[e] = 0.0;
        __syncthreads();
    }
    if (tid < NCB) {
        double acc = 0.0;
        if (tid < C)
            for (int i = 0; i < P; ++i) acc = fma(tile[i * NCB + tid], dw[i * NCB + tid], acc);
        bsh[tid] = tid < C ? p.logprior[(size_t)m * p.NC + tid] - 0.5 * acc : 0.0;
    }
    __syncthreads();

    // ---- 6. the test samples ----
    const int s0 = sl_clamp(p.tptr[m], 0, p.S);
    int t1 = sl_clamp(p.tptr[m + 1], s0, p.S);
    if (t1 - s0 > p.tmax) t1 = s0 + p.tmax;
    for (int sb = s0; sb < t1; sb += LDA_T) {
        const bool live = t1 - sb > tid;
        const int s = live ? sb + tid : sb;
        double acc[NCB];
#pragma unroll
        for (int c = 0; c < NCB; ++c) acc[c] = 0.0;
        for (int i = 0; i < P; i += LDA_SU) {                   // LDA_SU vertices' loads before the arithmetic of the first
            int vv[LDA_SU];
            float xx[LDA_SU];
#pragma unroll
            for (int q = 0; q < LDA_SU; ++q) vv[q] = vsh[min(i + q, P - 1)];
#pragma unroll
            for (int q = 0; q < LDA_SU; ++q) xx[q] = p.Xt[(size_t)max(vv[q], 0) * p.Sp + s];
#pragma unroll
            for (int q = 0; q < LDA_SU; ++q) {
                if (i + q < P) {
                    const double t = vv[q] >= 0 ? (double)xx[q] - msh[i + q] : 0.0;
#pragma unroll
                    for (int c = 0; c < NCB; ++c) acc[c] = fma(dw[(i + q) * NCB + c], t, acc[c]);
                }
            }
        }
        double best = 0.0;
        int pred = 0;
#pragma unroll
        for (int c = 0; c < NCB; ++c) {
            acc[c] = bsh[c] + acc[c];
            if (c < C && (c == 0 || acc[c] > best)) {
                best = acc[c];
                pred = c;
            }
        }
        if (live) {
            const size_t so = (size_t)sl_clamp(p.sorig[s], 0, p.S - 1);
            if (p.scores) {
#pragma unroll
                for (int c = 0; c < NCB; ++c)
                    if (c < C) p.scores[(so * C + c) * p.U + u] = acc[c];
            }
            if (p.predictions) p.predictions[so * p.U + u] = (uint8_t)pred;
        }
        const int gr = p.sgroup[s], y = p.slabel[s];
        sl_tally(p.correct, live && pred == y && (unsigned)gr < (unsigned)p.G ? gr * C + y : -1, p.U, u, lane);
    }
}

template <int PB>
static void lda_launch(const SlLda& p, int Ub, int NM, hipStream_t stream) {
    static char name[40];
    static const int named = snprintf(name, sizeof name, "searchlight_lda_kernel<%d>", PB);
    (void)named;
    note_dispatch(name);
    const dim3 grid((unsigned)Ub, (unsigned)NM);
    if (p.C <= LDA_NARROW)
        hipLaunchKernelGGL((searchlight_lda_kernel<PB, LDA_NARROW>), grid, dim3(LDA_T), 0, stream, p);
    else
        hipLaunchKernelGGL((searchlight_lda_kernel<PB, SL_CMAX>), grid, dim3(LDA_T), 0, stream, p);
}

}  // namespace chebgcn

using namespace chebgcn;

extern "C" int chebgcn_searchlight_lda_query(int what) {
    switch (what) {
        case 0: return LDA_T;               // threads of a workgroup: test samples of one scoring pass
        case 1: return LDA_PMAX;            // the longest row
        case 2: return LDA_TS;              // training samples of a residual tile
        case 3: return SL_CMAX;            // the largest number of classes
        case 4: return LDA_NB;              // blocks along a side of the covariance triangle: a thread owns (bucket / this)^2 elements
        case 5: return SL_NMAX;            // models of one call
        case 6: return SL_TILES;           // 64-sample tiles of a model's test samples
        case 7: return SL_GMAX;            // groups
        case 8: return LDA_NARROW;          // up to this many classes the class tables in LDS are this wide, query 3 beyond
        default:
            if (what > 100 && what <= 100 + LDA_PMAX) return lda_bucket(what - 100);       // the ball bucket of a row of what - 100
            return -1;
    }
}

extern "C" int chebgcn_searchlight_lda(const float* Xt, int S, int M, const int32_t* rowptr, const int32_t* colidx, int nnz, int U,
                                       const int32_t* centres, int Ub, int bucket, const int32_t* class_ptr, const int32_t* class_idx,
                                       int nidx, const int32_t* test_ptr, int tmax, int NM, int C, const double* par,
                                       const double* logprior, double shrinkage, const int32_t* sgroup, const int32_t* slabel,
                                       const int32_t* sorig, int G, int32_t* correct, double* scores, uint8_t* predictions,
                                       double* gamma_out, chebgcn_stream stream_) {
    CG_REQUIRE(Xt && rowptr && colidx && centres && class_ptr && class_idx && test_ptr && par && logprior && sgroup && slabel && sorig &&
                   correct, "searchlight_lda: NULL argument");
    CG_REQUIRE(S >= 1 && M >= 1 && S <= INT_MAX - 31 && nnz >= 1 && U >= 1 && Ub >= 1 && nidx >= 1 && tmax >= 1 && tmax <= S && NM >= 1 &&
                   C >= 2 && G >= 1 && bucket >= 1,
               "searchlight_lda: bad shape (S = %d, M = %d, nnz = %d, U = %d, Ub = %d, %d listed samples, tmax = %d, NM = %d, C = %d, "
               "G = %d, bucket = %d)", S, M, nnz, U, Ub, nidx, tmax, NM, C, G, bucket);
    CG_REQUIRE(shrinkage < 0.0 || (shrinkage >= LDA_SHRINK_MIN && shrinkage <= 1.0),
               "searchlight_lda: shrinkage = %g; served: [%g, 1], or negative for Ledoit-Wolf", shrinkage, LDA_SHRINK_MIN);
    const long long tiles = ((long long)tmax + 63) / 64;
    if (NM > SL_NMAX || C > SL_CMAX || G > SL_GMAX || tiles > SL_TILES || (bucket != 32 && bucket != 64 && bucket != 128))
        return fail(CHEBGCN_EUNSUPPORTED, "searchlight_lda: NM = %d, C = %d, G = %d, tmax = %d, bucket = %d; served: NM <= %d, C <= %d, "
                    "G <= %d, tmax <= %d, bucket 32, 64 or 128", NM, C, G, tmax, bucket, SL_NMAX, SL_CMAX, SL_GMAX, SL_TILES * 64);
    CG_REQUIRE((((uintptr_t)Xt | (uintptr_t)rowptr | (uintptr_t)colidx | (uintptr_t)centres | (uintptr_t)class_ptr | (uintptr_t)class_idx |
                 (uintptr_t)test_ptr | (uintptr_t)sgroup | (uintptr_t)slabel | (uintptr_t)sorig | (uintptr_t)correct) & 3) == 0 &&
                   (((uintptr_t)par | (uintptr_t)logprior | (uintptr_t)scores | (uintptr_t)gamma_out) & 7) == 0,
               "searchlight_lda: unaligned argument");
    const SlLda p{Xt, rowptr, colidx, centres, class_ptr, class_idx, test_ptr, par, logprior, sgroup, slabel, sorig, correct, scores,
                  predictions, gamma_out, shrinkage, S, plane_stride(S), M, nnz, U, nidx, tmax, C, chebgcn_searchlight_query(100 + C), G};
    hipStream_t stream = (hipStream_t)stream_;
    switch (bucket) {
        case 32: lda_launch<32>(p, Ub, NM, stream); break;
        case 64: lda_launch<64>(p, Ub, NM, stream); break;
        default: lda_launch<128>(p, Ub, NM, stream); break;
    }
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}
