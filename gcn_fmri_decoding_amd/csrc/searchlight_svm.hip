// Searchlight decoding with a linear SVM (searchlight.searchlight(classifier='svc')): every (training set, centre) pair gets its own
// one-vs-rest linear SVM, solved in the dual by coordinate descent on the n x n Gram matrix of the training samples.  The on-chip
// state depends on the number of training samples n <= SVM_NMAX = 128 and not at all on the length of the row, so rows of any
// length are served: parcels, the whole brain.  ONE WORKGROUP (256 threads) owns one (centre, model) pair from the patterns to the
// counts, and everything in between stays in LDS.  The model and its orders are stated once, in include/chebgcn.h.
//
// EVERY OPERATION IS A SEPARATE CORRECTLY ROUNDED float64 MULTIPLY, ADD OR DIVIDE: contraction is off for this file (the pragma
// below), so that searchlight_host's NumPy restatement agrees bit for bit.
//
// searchlight_svm_kernel<NB>: NB in {32, 64, 128} the sample bucket (a training set of n <= NB samples).  LDS: the packed lower
// triangle of K (NB (NB + 1) / 2 float64: 66 048 B at NB = 128), a stage of SVM_TV = 16 vertices' centred values of the NB training
// samples and of SVM_TC = 32 test samples (which holds the chunk's scores afterwards), K_sj of a chunk of 32 test samples
// [32][NB + 1], alpha_j t_j of every class [32][NB], the vertex numbers and means of a super-tile of 256 vertices, and a few rows
// of scalars.
//
//   0. The row (clamped; empty: the workgroup returns), the model's training list (clamped; n < 1 or n > NB: the workgroup returns
//      and touches nothing), the labels of its samples.
//   1. Centring and Gram matrix (svm_pass).  The row's vertices are streamed in ascending order, 16 a tile, 256 a super-tile.  Per
//      super-tile thread t forms m_v of vertex t: one chain over the list in list order, one division (the first read of the
//      vertices; eight loads are issued before their chain).  Per tile thread (sample, vertex) reads Xt coalesced over the samples
//      (the second read) and stores (double)x - m_v; the loads of the next tile are issued before the arithmetic of the current
//      one.  The triangle is cut into 16 x 16 blocks of TB x TB elements, TB = NB / 16; thread t < 136 owns block (bi >= bj) in
//      TB x TB registers and runs ONE CHAIN OVER THE VERTICES per element: a_ij = a_ij + x_i x_j.  qd_i = (K_ii + 1) + D.
//   2. The solve.  A wave takes a class, classes round-robin over the four waves; two classes: class 0 is solved and negated
//      (the problems are mirror images: the same Q, the same alpha, the same bits).  Lane l holds g_j and alpha_j for j = l,
//      l + 64: a coordinate step broadcasts g_i and alpha_i (readlane), every lane forms PG, a and delta redundantly, and then
//      g_j = g_j + (t_i t_j) (delta (K_ji + 1)) in every lane with column i of K from LDS -- no cross-lane sum.  The sweep's
//      max |PG| is a max: order-free.  No barrier inside the solve.
//   3. Scoring.  The model's test samples, 32 a chunk: K_sj of the chunk by streaming the row again in the same order (thread
//      (4 test samples, NB / 32 training samples) in registers), then thread (test sample, class):
//      f = (a = 0; a = a + (alpha_j t_j) (K_sj + 1), j in list order), the first maximal class, and the counts by sl_tally of
//      searchlight_common.h (ballot, one int32 atomic per distinct (group, label)).
// Every value is a function of (model, centre, the lists) alone: no float atomics, no order that depends on the launch.
// Compiler report and what bounds the kernel (the instructions of a coordinate step, not their latency): DESIGN 4.26.
// Nothing read from memory is an address or a trip count unchecked: row, list and test pointers are clamped, centre and model
// numbers outside their ranges end the workgroup, a sample number outside [0, S) is a row of zeros of the centred patterns and is
// not counted in n, a vertex outside [0, M) is a column of zeros, group and label numbers outside their ranges add nothing.
#pragma clang fp contract(off)
#include "searchlight_common.h"
#include "searchlight_ball.h"

namespace chebgcn {

constexpr int SVM_T = LDA_T;                // threads of a workgroup
constexpr int SVM_NMAX = 128;               // the largest training set
constexpr int SVM_TV = 16;                  // vertices of a tile
constexpr int SVM_TC = 32;                  // test samples of a chunk
constexpr int SVM_SUP = SVM_T;              // vertices of a super-tile: one mean per thread
constexpr int SVM_ITMAX = 100000;           // sweeps at most
constexpr int SVM_NBLK = LDA_NB;            // blocks along a side of the Gram triangle
constexpr int SVM_BLOCKS = SVM_NBLK * (SVM_NBLK + 1) / 2;

static inline int svm_bucket(int n) { return n < 1 || n > SVM_NMAX ? -1 : n <= 32 ? 32 : n <= 64 ? 64 : 128; }

struct SlSvm {
    const float* Xt;            // [M][Sp]
    const int32_t* rowptr;      // [U + 1]
    const int32_t* colidx;      // [nnz]
    const int32_t* centres;     // [Ub] rows of this launch
    const int32_t* models;      // [NMb] models of this launch
    const int32_t* lptr;        // [NM + 1]
    const int32_t* lidx;        // [nidx]
    const int32_t* tptr;        // [NM + 1]
    const int32_t* sgroup;      // [S]
    const int32_t* slabel;      // [S]
    const int32_t* sorig;       // [S]
    int32_t* correct;           // [G][C][U]
    double* scores;             // [S][C][U] or NULL
    uint8_t* predictions;       // [S][U] or NULL
    int32_t* sweeps;            // [NM][U] or NULL
    double* residual;           // [NM][U] or NULL
    double D, Ub, tol;          // 1 / (2 C) and +inf (squared hinge), or 0 and C (hinge)
    int max_iter;
    int S, Sp, M, nnz, U, nidx, tmax, NM, C, G;
};

__device__ __forceinline__ double svm_bcast(double v, int l) {         // l uniform in the wave
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// One pass over the row's P vertices in ascending order, tile by tile: the centred values of the nl training samples lsh (and,
// with TEST, of the ns test samples from ts0) go through LDS, and every element's chain receives one product per vertex:
// without TEST a (block (bi >= bj) of the Gram triangle, cov threads), with TEST b (4 test samples x NB / 32 training samples,
// every thread).  Called by all threads; begins and ends in a barrier.
template <int NB, bool TEST>
__device__ __forceinline__ void svm_pass(const SlSvm& p, int r0, int P, int nl, int nv, int ts0, int ns, const int* lsh, int* vsh,
                                         double* msh, double* tile, double* ttile, int tid, bool cov, int bi, int bj,
                                         double (&a)[NB / SVM_NBLK][NB / SVM_NBLK], double (&b)[4][NB / 32]) {
    constexpr int TB = NB / SVM_NBLK, JW = NB / 32;
    constexpr int ROWS = SVM_T / NB, NI = SVM_TV / ROWS;        // vertices a thread stages per tile
    constexpr int TROWS = SVM_T / SVM_TC, TNI = SVM_TV / TROWS;
    static_assert(SVM_T % NB == 0 && SVM_TV % ROWS == 0 && SVM_TV % TROWS == 0 && SVM_SUP % SVM_TV == 0, "thread maps");
    const int lj = tid % NB, lq = tid / NB;                     // training stage: its sample, its first vertex
    const int pos = lj < nl ? lsh[lj] : -1;
    const int tss = tid % SVM_TC, tsq = tid / SVM_TC;           // test stage
    const int tpos = TEST && tss < ns ? ts0 + tss : -1;
    const int sb4 = (tid / 32) * 4, jb = (tid % 32) * JW;       // its block of b
    float xr[NI], xt[TNI];
    unsigned live = 0, tlive = 0;                               // bit q: xr[q] / xt[q] is a value

    auto setup = [&](int v0) {                                  // the super-tile from row entry v0: vertex numbers and means
        const int i = v0 + tid;
        int v = i < P ? p.colidx[r0 + i] : -1;
        if ((unsigned)v >= (unsigned)p.M) v = -1;
        vsh[tid] = v;
        double acc = 0.0;
        if (v >= 0) {
            const float* row = p.Xt + (size_t)v * p.Sp;
            int k = 0;
            for (; k + 8 <= nl; k += 8) {
                float x[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int s = lsh[k + q];
                    x[q] = s >= 0 ? row[s] : 0.0f;
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) acc = acc + (double)x[q];
            }
            for (; k < nl; ++k) {
                const int s = lsh[k];
                acc = acc + (double)(s >= 0 ? row[s] : 0.0f);
            }
        }
        msh[tid] = nv ? acc / (double)nv : 0.0;
    };
    auto fetch = [&](int t) {
        const int base = (t * SVM_TV) % SVM_SUP;
        live = 0;
#pragma unroll
        for (int q = 0; q < NI; ++q) {
            const int qq = lq + q * ROWS;
            const int v = t * SVM_TV + qq < P ? vsh[base + qq] : -1;
            xr[q] = 0.0f;
            if (pos >= 0 && v >= 0) {
                xr[q] = p.Xt[(size_t)v * p.Sp + pos];
                live |= 1u << q;
            }
        }
        if (TEST) {
            tlive = 0;
#pragma unroll
            for (int q = 0; q < TNI; ++q) {
                const int qq = tsq + q * TROWS;
                const int v = t * SVM_TV + qq < P ? vsh[base + qq] : -1;
                xt[q] = 0.0f;
                if (tpos >= 0 && v >= 0) {
                    xt[q] = p.Xt[(size_t)v * p.Sp + tpos];
                    tlive |= 1u << q;
                }
            }
        }
    };

    const int tiles = (P + SVM_TV - 1) / SVM_TV;
    __syncthreads();
    setup(0);
    __syncthreads();
    fetch(0);
    for (int t = 0; t < tiles; ++t) {
        const int base = (t * SVM_TV) % SVM_SUP;
#pragma unroll
        for (int q = 0; q < NI; ++q) {
            const int qq = lq + q * ROWS;
            tile[qq * NB + lj] = live >> q & 1 ? (double)xr[q] - msh[base + qq] : 0.0;
        }
        if (TEST) {
#pragma unroll
            for (int q = 0; q < TNI; ++q) {
                const int qq = tsq + q * TROWS;
                ttile[qq * SVM_TC + tss] = tlive >> q & 1 ? (double)xt[q] - msh[base + qq] : 0.0;
            }
        }
        const int kn = min(SVM_TV, P - t * SVM_TV);
        __syncthreads();
        if (t + 1 < tiles) {
            if ((t + 1) * SVM_TV % SVM_SUP == 0) {              // (nobody reads vsh or msh between the barrier above and the next)
                setup((t + 1) * SVM_TV);
                __syncthreads();
            }
            fetch(t + 1);
        }
        if (!TEST) {
            if (cov) {
                for (int q = 0; q < kn; ++q) {
                    double ri[TB], rj[TB];
#pragma unroll
                    for (int x = 0; x < TB; ++x) ri[x] = tile[q * NB + bi * TB + x];
#pragma unroll
                    for (int x = 0; x < TB; ++x) rj[x] = tile[q * NB + bj * TB + x];
#pragma unroll
                    for (int x = 0; x < TB; ++x)
#pragma unroll
                        for (int y = 0; y < TB; ++y) a[x][y] = a[x][y] + ri[x] * rj[y];
                }
            }
        } else if (sb4 < ns && jb < nl) {
            for (int q = 0; q < kn; ++q) {
                double ts[4], tr[JW];
#pragma unroll
                for (int x = 0; x < 4; ++x) ts[x] = ttile[q * SVM_TC + sb4 + x];
#pragma unroll
                for (int y = 0; y < JW; ++y) tr[y] = tile[q * NB + jb + y];
#pragma unroll
                for (int x = 0; x < 4; ++x)
#pragma unroll
                    for (int y = 0; y < JW; ++y) b[x][y] = b[x][y] + ts[x] * tr[y];
            }
        }
        __syncthreads();
    }
}

// block (centre blockIdx.x of the launch, model blockIdx.y of the launch)
template <int NB>
__global__ void __launch_bounds__(SVM_T)
searchlight_svm_kernel(SlSvm p) {
    constexpr int TB = NB / SVM_NBLK, JW = NB / 32, NJ = NB > 64 ? NB / 64 : 1, LDK = NB + 1;
    static_assert(SVM_TV * (NB + SVM_TC) >= SVM_TC * SL_CMAX, "the stage holds the chunk's scores");
    static_assert(SVM_BLOCKS <= SVM_T && NB <= SVM_T && SVM_T / 64 == 4, "thread maps");
    __shared__ double Ksh[NB * (NB + 1) / 2];                   // K: element (i >= j) at i (i + 1) / 2 + j
    __shared__ double stage[SVM_TV * (NB + SVM_TC)];            // [q][j] training, then [q][s] test; afterwards scores [c][s]
    __shared__ double Kte[SVM_TC * LDK];                        // [s][j] of the chunk
    __shared__ double ash[SL_CMAX * NB];                       // [c][j]: alpha_j t_j
    __shared__ double msh[SVM_SUP];
    __shared__ double qd[NB];
    __shared__ double rssh[SL_CMAX];
    __shared__ int vsh[SVM_SUP];
    __shared__ int lsh[NB];                                     // the training samples, -1: outside [0, S)
    __shared__ int ysh[NB];                                     // their labels
    __shared__ int swsh[SL_CMAX];
    __shared__ int nvsh;
    double* const tile = stage;
    double* const ttile = stage + SVM_TV * NB;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int u = p.centres[blockIdx.x];
    const int m = p.models[blockIdx.y];
    if ((unsigned)u >= (unsigned)p.U || (unsigned)m >= (unsigned)p.NM) return;
    const int r0 = sl_clamp(p.rowptr[u], 0, p.nnz), r1 = sl_clamp(p.rowptr[u + 1], r0, p.nnz);
    const int P = r1 - r0;
    const int l0 = sl_clamp(p.lptr[m], 0, p.nidx), l1 = sl_clamp(p.lptr[m + 1], l0, p.nidx);
    const int nl = l1 - l0;
    if (P < 1 || nl < 1 || nl > NB) return;
    const int C = p.C;                                          // 2 <= C <= 32: the entry point's check

    // ---- 0. the training list ----
    if (tid < NB) {
        int s = tid < nl ? p.lidx[l0 + tid] : -1;
        if ((unsigned)s >= (unsigned)p.S) s = -1;
        lsh[tid] = s;
        ysh[tid] = s >= 0 ? p.slabel[s] : -1;
    }
    __syncthreads();
    if (tid == 0) {
        int nv = 0;
        for (int i = 0; i < nl; ++i) nv += lsh[i] >= 0;
        nvsh = nv;
    }
    __syncthreads();
    const int nv = nvsh;

    // ---- 1. centring and Gram matrix ----
    {
        int bi, bj;
        ball_block(tid, bi, bj);
        const bool cov = tid < SVM_BLOCKS && bi * TB < nl;
        double a[TB][TB], b0[4][JW];
#pragma unroll
        for (int x = 0; x < TB; ++x)
#pragma unroll
            for (int y = 0; y < TB; ++y) a[x][y] = 0.0;
        svm_pass<NB, false>(p, r0, P, nl, nv, 0, 0, lsh, vsh, msh, tile, ttile, tid, cov, bi, bj, a, b0);
        if (cov) {
#pragma unroll
            for (int x = 0; x < TB; ++x)
#pragma unroll
                for (int y = 0; y < TB; ++y) {
                    const int i = bi * TB + x, j = bj * TB + y;
                    if (i < nl && j <= i) Ksh[i * (i + 1) / 2 + j] = a[x][y];
                }
        }
        __syncthreads();
        if (tid < nl) qd[tid] = (Ksh[tid * (tid + 1) / 2 + tid] + 1.0) + p.D;
        __syncthreads();
    }

    // ---- 2. the solve: a wave a class ----
    {
        const double D = p.D, Ub = p.Ub, tol = p.tol;
        const int solved = C == 2 ? 1 : C;
        for (int c = tid >> 6; c < solved; c += SVM_T / 64) {
            double g[NJ], al[NJ], tj[NJ];
#pragma unroll
            for (int r = 0; r < NJ; ++r) {
                const int j = lane + 64 * r;
                g[r] = -1.0;
                al[r] = 0.0;
                tj[r] = j < nl && ysh[j] == c ? 1.0 : -1.0;
            }
            int done = 0;
            double res = 0.0;
            for (int e = 1; e <= p.max_iter; ++e) {
                double mx = 0.0;
                for (int i = 0; i < nl; ++i) {
                    const int src = i & 63;
                    double gs = g[0], as = al[0];
                    if (NJ > 1 && i >= 64) {
                        gs = g[NJ - 1];
                        as = al[NJ - 1];
                    }
                    const double G = svm_bcast(gs, src), ai = svm_bcast(as, src);
                    const double ti = ysh[i] == c ? 1.0 : -1.0;
                    double PG = G;
                    if (ai == 0.0)
                        PG = fmin(G, 0.0);
                    else if (ai == Ub)
                        PG = fmax(G, 0.0);
                    if (PG != 0.0) {
                        const double an = fmin(fmax(ai - G / qd[i], 0.0), Ub);
                        const double delta = an - ai;
#pragma unroll
                        for (int r = 0; r < NJ; ++r) {
                            const int j = lane + 64 * r;
                            if (j < nl) {
                                const double q = Ksh[j >= i ? j * (j + 1) / 2 + i : i * (i + 1) / 2 + j] + 1.0;
                                g[r] = g[r] + (ti * tj[r]) * (delta * q);
                                if (j == i) {
                                    g[r] = g[r] + delta * D;
                                    al[r] = an;
                                }
                            }
                        }
                    }
                    mx = fmax(mx, fabs(PG));
                }
                done = e;
                res = mx;
                if (mx <= tol) break;
            }
#pragma unroll
            for (int r = 0; r < NJ; ++r) {
                const int j = lane + 64 * r;
                if (j < NB) {
                    const double at = j < nl ? al[r] * tj[r] : 0.0;
                    ash[c * NB + j] = at;
                    if (C == 2) ash[NB + j] = -at;
                }
            }
            if (lane == 0) {
                swsh[c] = done;
                rssh[c] = res;
                if (C == 2) {
                    swsh[1] = done;
                    rssh[1] = res;
                }
            }
        }
        __syncthreads();
        if (tid == 0 && (p.sweeps || p.residual)) {
            int sw = 0;
            double rs = 0.0;
            for (int c = 0; c < C; ++c) {
                sw = max(sw, swsh[c]);
                rs = fmax(rs, rssh[c]);
            }
            if (p.sweeps) p.sweeps[(size_t)m * p.U + u] = sw;
            if (p.residual) p.residual[(size_t)m * p.U + u] = rs;
        }
    }

    // ---- 3. the test samples, a chunk at a time ----
    const int s0 = sl_clamp(p.tptr[m], 0, p.S);
    int t1 = sl_clamp(p.tptr[m + 1], s0, p.S);
    if (t1 - s0 > p.tmax) t1 = s0 + p.tmax;
    for (int sb = s0; sb < t1; sb += SVM_TC) {
        const int ns = min(SVM_TC, t1 - sb);
        {
            double a0[TB][TB], b[4][JW];
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < JW; ++y) b[x][y] = 0.0;
            svm_pass<NB, true>(p, r0, P, nl, nv, sb, ns, lsh, vsh, msh, tile, ttile, tid, false, 0, 0, a0, b);
            const int sb4 = (tid / 32) * 4, jb = (tid % 32) * JW;
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < JW; ++y)
                    if (sb4 + x < ns && jb + y < nl) Kte[(sb4 + x) * LDK + jb + y] = b[x][y];
        }
        __syncthreads();
        double* const scsh = stage;                             // [c][s]: the pass is over, its stage is free
        for (int e = tid; e < SVM_TC * C; e += SVM_T) {
            const int s = e % SVM_TC, c = e / SVM_TC;
            if (s < ns) {
                double acc = 0.0;
                for (int j = 0; j < nl; ++j) acc = acc + ash[c * NB + j] * (Kte[s * LDK + j] + 1.0);
                scsh[c * SVM_TC + s] = acc;
            }
        }
        __syncthreads();
        if (tid < 64) {
            const bool live = tid < ns;
            const int s = live ? sb + tid : sb;
            double best = 0.0;
            int pred = 0;
            if (live) {
                for (int c = 0; c < C; ++c) {
                    const double f = scsh[c * SVM_TC + tid];
                    if (c == 0 || f > best) {
                        best = f;
                        pred = c;
                    }
                }
                const size_t so = (size_t)sl_clamp(p.sorig[s], 0, p.S - 1);
                if (p.scores)
                    for (int c = 0; c < C; ++c) p.scores[(so * C + c) * p.U + u] = scsh[c * SVM_TC + tid];
                if (p.predictions) p.predictions[so * p.U + u] = (uint8_t)pred;
            }
            const int gr = p.sgroup[s], y = p.slabel[s];
            sl_tally(p.correct, live && pred == y && (unsigned)gr < (unsigned)p.G ? gr * C + y : -1, p.U, u, lane);
        }
        // (the next pass begins with a barrier: the scores are read before the stage is written again)
    }
}

template <int NB>
static void svm_launch(const SlSvm& p, int Ub, int NMb, hipStream_t stream) {
    static char name[40];
    static const int named = snprintf(name, sizeof name, "searchlight_svm_kernel<%d>", NB);
    (void)named;
    note_dispatch(name);
    hipLaunchKernelGGL((searchlight_svm_kernel<NB>), dim3((unsigned)Ub, (unsigned)NMb), dim3(SVM_T), 0, stream, p);
}

}  // namespace chebgcn

using namespace chebgcn;

extern "C" int chebgcn_searchlight_svm_query(int what) {
    switch (what) {
        case 0: return SVM_T;               // threads of a workgroup
        case 1: return SVM_NMAX;            // the largest training set
        case 2: return SVM_TV;              // vertices of a tile
        case 3: return SL_CMAX;            // the largest number of classes
        case 4: return SVM_TC;              // test samples of a chunk
        case 5: return SL_NMAX;          // models of one call
        case 6: return SL_TILES;           // 64-sample tiles of a model's test samples
        case 7: return SL_GMAX;            // groups
        case 8: return SVM_ITMAX;           // sweeps at most
        case 9: return SVM_SUP;             // vertices of a super-tile
        default:
            if (what > 100 && what <= 100 + SVM_NMAX) return svm_bucket(what - 100);       // the bucket of a training set of what - 100
            return -1;
    }
}

extern "C" int chebgcn_searchlight_svm(const float* Xt, int S, int M, const int32_t* rowptr, const int32_t* colidx, int nnz, int U,
                                       const int32_t* centres, int Ub, const int32_t* models, int NMb, int bucket,
                                       const int32_t* list_ptr, const int32_t* list_idx, int nidx, const int32_t* test_ptr, int tmax,
                                       int NM, int C, double Creg, int loss, double tol, int max_iter, const int32_t* sgroup,
                                       const int32_t* slabel, const int32_t* sorig, int G, int32_t* correct, double* scores,
                                       uint8_t* predictions, int32_t* sweeps, double* residual, chebgcn_stream stream_) {
    CG_REQUIRE(Xt && rowptr && colidx && centres && models && list_ptr && list_idx && test_ptr && sgroup && slabel && sorig && correct,
               "searchlight_svm: NULL argument");
    CG_REQUIRE(S >= 1 && M >= 1 && S <= INT_MAX - 31 && nnz >= 1 && U >= 1 && Ub >= 1 && NMb >= 1 && nidx >= 1 && tmax >= 1 && tmax <= S &&
                   NM >= 1 && C >= 2 && G >= 1 && bucket >= 1,
               "searchlight_svm: bad shape (S = %d, M = %d, nnz = %d, U = %d, Ub = %d, NMb = %d, %d listed samples, tmax = %d, NM = %d, "
               "C = %d, G = %d, bucket = %d)", S, M, nnz, U, Ub, NMb, nidx, tmax, NM, C, G, bucket);
    CG_REQUIRE(Creg > 0.0 && Creg <= DBL_MAX, "searchlight_svm: C = %g; served: finite and > 0", Creg);
    CG_REQUIRE(tol >= 0.0 && tol <= DBL_MAX, "searchlight_svm: tol = %g; served: finite and >= 0", tol);
    CG_REQUIRE(loss == 0 || loss == 1, "searchlight_svm: loss = %d; served: 0 (squared hinge) or 1 (hinge)", loss);
    CG_REQUIRE(max_iter >= 1 && max_iter <= SVM_ITMAX, "searchlight_svm: max_iter = %d; served: 1 .. %d", max_iter, SVM_ITMAX);
    const long long tiles = ((long long)tmax + 63) / 64;
    if (NM > SL_NMAX || NMb > SL_NMAX || C > SL_CMAX || G > SL_GMAX || tiles > SL_TILES ||
        (bucket != 32 && bucket != 64 && bucket != 128))
        return fail(CHEBGCN_EUNSUPPORTED, "searchlight_svm: NM = %d, NMb = %d, C = %d, G = %d, tmax = %d, bucket = %d; served: NM <= %d, "
                    "C <= %d, G <= %d, tmax <= %d, bucket 32, 64 or 128", NM, NMb, C, G, tmax, bucket, SL_NMAX, SL_CMAX, SL_GMAX,
                    SL_TILES * 64);
    CG_REQUIRE((((uintptr_t)Xt | (uintptr_t)rowptr | (uintptr_t)colidx | (uintptr_t)centres | (uintptr_t)models | (uintptr_t)list_ptr |
                 (uintptr_t)list_idx | (uintptr_t)test_ptr | (uintptr_t)sgroup | (uintptr_t)slabel | (uintptr_t)sorig |
                 (uintptr_t)correct | (uintptr_t)sweeps) & 3) == 0 && (((uintptr_t)scores | (uintptr_t)residual) & 7) == 0,
               "searchlight_svm: unaligned argument");
    const double D = loss == 0 ? 1.0 / (2.0 * Creg) : 0.0;
    const double Ubound = loss == 0 ? (double)INFINITY : Creg;
    const SlSvm p{Xt, rowptr, colidx, centres, models, list_ptr, list_idx, test_ptr, sgroup, slabel, sorig, correct, scores, predictions,
                  sweeps, residual, D, Ubound, tol, max_iter, S, plane_stride(S), M, nnz, U, nidx, tmax, NM, C, G};
    hipStream_t stream = (hipStream_t)stream_;
    switch (bucket) {
        case 32: svm_launch<32>(p, Ub, NMb, stream); break;
        case 64: svm_launch<64>(p, Ub, NMb, stream); break;
        default: svm_launch<128>(p, Ub, NMb, stream); break;
    }
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}
