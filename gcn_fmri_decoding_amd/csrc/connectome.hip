// Functional connectivity matrices per run (connectome.connectome): the Ledoit-Wolf (or fixed) shrunk covariance of a run's
// regions, its correlation, its inverse (the precision) and the partial correlation, all in float64 from the staged float32
// planes, rounded once.  include/chebgcn.h states the arithmetic and the order of every sum; DESIGN 4.33 tells why each choice.
//
// Per run a workspace of cn_ws_doubles(Rp) doubles: the matrix [Rp][Rp] (row stride Rp), then four vectors of Rp: the region means, the
// reciprocal Cholesky diagonal, the diagonal of the precision, and the scalars {beta_, shrinkage, degenerate}.
//
//   connectome_centre_kernel   thread (run, region): the mean, one chain over ascending t.
//   connectome_rowsq_kernel    workgroup = run, 8 waves: wave w takes rows t0 + w, t0 + w + 8, ...; q_t = sum_i d_ti^2 is a chain
//                              per lane over i = lane, lane + 64, ... and a butterfly over the lanes; the wave sums q_t^2 over its
//                              rows in ascending t, and the eight sums are added in ascending w.  A function of (T, R) alone.
//   connectome_cov_kernel      workgroup (lower-triangle tile of 64 x 64, run), 256 threads, a thread owns 4 x 4 float64
//                              accumulators: the deviations of CN_TK rows of the two column panels go to LDS as float64 (pad
//                              columns and rows beyond the run as 0, whatever the memory holds), every thread reads 4 + 4 of them
//                              per row for 16 FMAs.  An accumulator is ONE chain fma(d_ti, d_tj, acc) over ascending t of the run:
//                              a run is never cut along time (S runs x 21 tiles at R = 360 fill the part without it), so there is
//                              no slice rule to state.  A diagonal tile forms (i, j) and (j, i) from the same products in the same
//                              order; an off-diagonal tile writes its value to both places: C is symmetric bit for bit.
//                              Vector FMA, not v_mfma_f64_16x16x4_f64: the matrix instruction runs at the same float64 rate on
//                              this part, what it could save is LDS reads, and its accumulation order inside the instruction is
//                              not ours to state -- the chain above is.
//   connectome_finish_kernel<INV>  workgroup = run, 512 threads.  delta_ and the trace by fixed trees, the shrinkage, Sigma in
//                              place; without INV the covariance / correlation go out from here.  With INV, thread i = row i:
//                              a left-looking blocked Cholesky, panels of CN_NB columns held in registers (16 accumulators), the
//                              finished columns read back coalesced from the workspace (column p of L = row p of the matrix,
//                              strictly above the diagonal) and the CN_NB entries every thread needs of them broadcast from an LDS
//                              panel of CN_PB x CN_NB doubles; the diagonal block is eliminated inside its wave by cross-lane
//                              moves, the rows below take it from LDS.  Every entry is ONE chain over ascending p.
//   connectome_invert_kernel   workgroup = run, 512 threads, thread c = column c of M = L^-1 by forward substitution in the same
//                              blocking (16 rows of the column in registers), M stored on and below the diagonal of the same
//                              matrix (the diagonal of L lives on as its reciprocal in a vector); then the diagonal of P.  A
//                              kernel of its own so that each of the two has its registers to itself (101 and 83 VGPRs, no
//                              scratch; one kernel for both spilt).
//   connectome_gram_kernel     P = M^T M on the tiles and with the body of the covariance kernel (rows p >= the tile's first row,
//                              entries above the diagonal of M read as 0), normalised, mirrored, rounded once.
//   connectome_mean_kernel     thread = entry: float64 sum of the float32 matrices of the runs that are not flagged, ascending.
// No float atomics.  Run offsets are clamped into [0, Ttot]; nothing read from memory is an address unchecked.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "glm_pass.h"

namespace chebgcn {

constexpr int CN_RMAX = 512;                // regions: one row per thread of a finish workgroup
constexpr int CN_SMAX = 65535;              // runs of one call (grid.y)
constexpr int CN_TILE = 64;                 // a covariance / gram tile is CN_TILE x CN_TILE
constexpr int CN_TK = 16;                   // rows of a tile's operands in LDS at once
constexpr int CN_CT = 256;                  // threads of a tile workgroup: 16 x 16, 4 x 4 entries each
constexpr int CN_FT = 512;                  // threads of a finish workgroup
constexpr int CN_NB = 16;                   // columns of a Cholesky panel = accumulators of a thread
constexpr int CN_PB = 64;                   // finished columns staged in LDS at once
constexpr int CN_QW = 8;                    // waves of a rowsq workgroup
constexpr int CN_MT = 256;                  // threads of centre / mean

__host__ __device__ constexpr size_t cn_ws_doubles(int Rp) { return (size_t)Rp * Rp + 4 * (size_t)Rp; }

struct CnRun {
    double* A;          // [Rp][Rp]
    double* mean;       // [Rp]
    double* dinv;       // [Rp]
    double* pdiag;      // [Rp]
    double* scal;       // [Rp]: 0 beta_, 1 shrinkage, 2 degenerate (0 / 1)
};
__device__ __forceinline__ CnRun cn_run(double* ws, int r, int Rp) {
    double* A = ws + (size_t)r * cn_ws_doubles(Rp);
    double* v = A + (size_t)Rp * Rp;
    return CnRun{A, v, v + Rp, v + 2 * Rp, v + 3 * Rp};
}

// thread (region m < Rp, run blockIdx.y)
__global__ void __launch_bounds__(CN_MT)
connectome_centre_kernel(const float* __restrict__ series, long long Ttot, const long long* __restrict__ offs, int R, int Rp,
                         double* __restrict__ ws) {
    const int m = blockIdx.x * CN_MT + threadIdx.x;
    const int r = blockIdx.y;
    if (m >= Rp) return;
    long long t0, t1;
    glm_run(offs, r, Ttot, t0, t1);
    double acc = 0.0;
    if (m < R) {
#pragma unroll 4
        for (long long t = t0; t < t1; ++t) acc = acc + (double)series[(size_t)t * Rp + m];
    }
    cn_run(ws, r, Rp).mean[m] = t1 > t0 && m < R ? acc / (double)(t1 - t0) : 0.0;
}

// workgroup = run
__global__ void __launch_bounds__(CN_QW * 64)
connectome_rowsq_kernel(const float* __restrict__ series, long long Ttot, const long long* __restrict__ offs, int R, int Rp,
                        double* __restrict__ ws) {
    __shared__ double part[CN_QW];
    const int r = blockIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const CnRun run = cn_run(ws, r, Rp);
    long long t0, t1;
    glm_run(offs, r, Ttot, t0, t1);
    double mu[CN_RMAX / 64];
#pragma unroll
    for (int u = 0; u < CN_RMAX / 64; ++u) mu[u] = lane + 64 * u < R ? run.mean[lane + 64 * u] : 0.0;
    double b = 0.0;
    for (long long t = t0 + w; t < t1; t += CN_QW) {
        const float* row = series + (size_t)t * Rp;
        double q = 0.0;
#pragma unroll
        for (int u = 0; u < CN_RMAX / 64; ++u) {
            const int i = lane + 64 * u;
            if (i < R) {
                const double d = (double)row[i] - mu[u];
                q = fma(d, d, q);
            }
        }
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) q = q + __shfl_xor(q, s, 64);
        b = fma(q, q, b);
    }
    if (lane == 0) part[w] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = part[0];
        for (int u = 1; u < CN_QW; ++u) s = s + part[u];
        run.scal[0] = s;
    }
}

// The body the covariance and the gram kernel share: acc[i][j] = fma(a[t][ca + 4 ty + i], b[t][cb + 4 tx + j], acc[i][j]) over
// ascending t in [ta, tb), CN_TK rows through LDS at a time.  load(t, col, v) gives columns col .. col + 3 of row t as float64
// (0 outside the operand); every thread of the workgroup calls this (it holds barriers)
template <class Load>
__device__ __forceinline__ void cn_tile(double (&acc)[4][4], long long ta, long long tb, int ca, int cb, Load load,
                                        double (*As)[CN_TILE], double (*Bs)[CN_TILE]) {
    const int tid = threadIdx.x, lr = tid >> 4, lc = (tid & 15) * 4;
    const int ty = tid >> 4, tx = tid & 15;
    const bool diag = ca == cb;
    double(*Bu)[CN_TILE] = diag ? As : Bs;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    for (long long tc = ta; tc < tb; tc += CN_TK) {
        double va[4], vb[4];
        load(tc + lr, ca + lc, va);
        if (!diag) load(tc + lr, cb + lc, vb);
#pragma unroll
        for (int v = 0; v < 4; ++v) As[lr][lc + v] = va[v];
        if (!diag) {
#pragma unroll
            for (int v = 0; v < 4; ++v) Bs[lr][lc + v] = vb[v];
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < CN_TK; ++k) {
            double a[4], b[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                a[v] = As[k][ty * 4 + v];
                b[v] = Bu[k][tx * 4 + v];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
}

// tile x of the lower triangle, row-major: (bi, bj), bj <= bi
__device__ __forceinline__ void cn_tile_of(int x, int& bi, int& bj) {
    bi = 0;
    while ((bi + 1) * (bi + 2) / 2 <= x) ++bi;
    bj = x - bi * (bi + 1) / 2;
}

// block (tile blockIdx.x, run blockIdx.y)
__global__ void __launch_bounds__(CN_CT)
connectome_cov_kernel(const float* __restrict__ series, long long Ttot, const long long* __restrict__ offs, int R, int Rp,
                      double* __restrict__ ws) {
    __shared__ double As[CN_TK][CN_TILE], Bs[CN_TK][CN_TILE];
    const int r = blockIdx.y;
    int bi, bj;
    cn_tile_of((int)blockIdx.x, bi, bj);
    const CnRun run = cn_run(ws, r, Rp);
    long long t0, t1;
    glm_run(offs, r, Ttot, t0, t1);
    const double* mean = run.mean;
    // a vector of four columns lies inside the row or beyond it (Rp is a multiple of 32); one beyond it reads the row's first
    // vector and drops it, as a row beyond the run reads the last row of the planes
    auto load = [&](long long t, int col, double (&v)[4]) {
        const long long tr = min(max(t, 0LL), Ttot - 1);
        const int cc = col < Rp ? col : 0;
        const float4 x = *reinterpret_cast<const float4*>(series + (size_t)tr * Rp + cc);
        const double m0 = mean[cc], m1 = mean[cc + 1], m2 = mean[cc + 2], m3 = mean[cc + 3];
        const bool in = t < t1;
        v[0] = in && col + 0 < R ? (double)x.x - m0 : 0.0;
        v[1] = in && col + 1 < R ? (double)x.y - m1 : 0.0;
        v[2] = in && col + 2 < R ? (double)x.z - m2 : 0.0;
        v[3] = in && col + 3 < R ? (double)x.w - m3 : 0.0;
    };
    double acc[4][4];
    cn_tile(acc, t0, t1, bi * CN_TILE, bj * CN_TILE, load, As, Bs);
    const double T = (double)(t1 - t0);
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gi = bi * CN_TILE + ty * 4 + i, gj = bj * CN_TILE + tx * 4 + j;
            if (gi >= R || gj >= R) continue;
            const double c = t1 > t0 ? acc[i][j] / T : 0.0;
            run.A[(size_t)gi * Rp + gj] = c;
            if (bi != bj) run.A[(size_t)gj * Rp + gi] = c;
        }
}

struct CnFinish {
    double* ws;
    const long long* offs;      // [S + 1]
    long long Ttot;
    int R, Rp, kind;
    double shrinkage;           // < 0: Ledoit-Wolf
    float* out;                 // [S][R][R]
    double* shrink_out;         // [S]
    int32_t* degenerate;        // [S]
};

// the sum of the workgroup's CN_FT values, by the same tree whatever they are; every thread calls it and gets the sum
__device__ __forceinline__ double cn_block_sum(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = CN_FT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// Ls[pp][j] = A[p0 + pp][c0 + j] = L[c0 + j][p0 + pp] for the rows p0 + pp < pend, 0 beyond (c0 + CN_NB <= Rp: c0 is a multiple
// of CN_NB below R and Rp a multiple of 32).  Barriers on both sides belong to the caller
__device__ __forceinline__ void cn_stage(const double* A, int Rp, int p0, int pend, int c0, double (*Ls)[CN_NB]) {
#pragma unroll
    for (int u = 0; u < CN_PB * CN_NB / CN_FT; ++u) {
        const int idx = (int)threadIdx.x + CN_FT * u, pp = idx / CN_NB, j = idx % CN_NB;
        Ls[pp][j] = p0 + pp < pend ? A[(size_t)(p0 + pp) * Rp + c0 + j] : 0.0;
    }
}

// delta = ((delta_ - (2 mu) tr) + (R mu) mu) / R with every operation rounded on its own: for one region (and wherever C is a
// multiple of the identity) the three terms cancel to exactly 0 and the shrinkage is 0; fused, the products keep their low bits,
// delta is a round-off residue above 0 and the shrinkage 1 (measured at R = 1)
__device__ __forceinline__ double cn_delta(double delta_, double mu, double tr, double Rd) {
#pragma clang fp contract(off)
    const double a = (2.0 * mu) * tr;
    const double b = (Rd * mu) * mu;
    return ((delta_ - a) + b) / Rd;
}

// The CN_NB accumulators of a thread.  A vector and not an array: the eliminations inside a diagonal block run column by column in
// a loop that is NOT unrolled (unrolled, the compiler reads all 120 entries of the block ahead of the first column and spills:
// 292 bytes of scratch a lane, measured), and the entry of a column that is not a constant then comes out of the registers
typedef double cn_acc __attribute__((ext_vector_type(CN_NB)));

// The shrinkage of run r and Sigma = (1 - s) C + s mu I in place of C, for the finish and the sigma kernel alike (one body: the
// float64 Sigma of chebgcn_connectome_sigma rounds to the bits of the covariance kind).  Every thread of a CN_FT workgroup calls
// it (it holds barriers) and gets the shrinkage; thread 0 stores it
__device__ __forceinline__ double cn_shrink(const CnFinish& p, int r, const CnRun& run, double* red) {
    const int tid = threadIdx.x;
    const int R = p.R, Rp = p.Rp;
    double* A = run.A;
    long long t0, t1;
    glm_run(p.offs, r, p.Ttot, t0, t1);
    const double T = (double)(t1 - t0), Rd = (double)R;

    // delta_ = sum_ij C_ij^2 and the trace
    double part = 0.0;
    for (int e = tid; e < R * R; e += CN_FT) {
        const int i = e / R, j = e - i * R;
        const double v = A[(size_t)i * Rp + j];
        part = fma(v, v, part);
    }
    const double delta_ = cn_block_sum(part, red);
    const double tr = cn_block_sum(tid < R ? A[(size_t)tid * Rp + tid] : 0.0, red);
    const double mu = tr / Rd;
    double s = p.shrinkage;
    if (s < 0.0) {
        const double beta = t1 > t0 ? (run.scal[0] / T - delta_) / (Rd * T) : 0.0;
        const double delta = cn_delta(delta_, mu, tr, Rd);
        double b = beta < delta ? beta : delta;
        b = b > 0.0 ? b : 0.0;
        s = delta > 0.0 ? b / delta : 0.0;
    }
    // Sigma = (1 - s) C + s mu I, in place
    const double keep = 1.0 - s, lift = s * mu;
    for (int e = tid; e < R * R; e += CN_FT) {
        const int i = e / R, j = e - i * R;
        const size_t o = (size_t)i * Rp + j;
        A[o] = fma(keep, A[o], i == j ? lift : 0.0);
    }
    if (tid == 0) {
        p.shrink_out[r] = s;
        run.scal[1] = s;
    }
    __syncthreads();
    return s;
}

// workgroup = run: Sigma in float64, dense [R][R] (chebgcn_connectome_sigma; p.out is not used)
__global__ void __launch_bounds__(CN_FT)
connectome_sigma_kernel(CnFinish p, double* __restrict__ sigma) {
    __shared__ double red[CN_FT];
    const int r = blockIdx.x, R = p.R;
    const CnRun run = cn_run(p.ws, r, p.Rp);
    cn_shrink(p, r, run, red);
    double* out = sigma + (size_t)r * R * R;
    for (int e = threadIdx.x; e < R * R; e += CN_FT) {
        const int i = e / R, j = e - i * R;
        out[e] = run.A[(size_t)i * p.Rp + j];
    }
}

// workgroup = run
template <bool INV>
__global__ void __launch_bounds__(CN_FT)
connectome_finish_kernel(CnFinish p) {
    __shared__ double red[CN_FT];
    __shared__ double Ls[CN_PB][CN_NB];
    __shared__ double Ld[CN_NB][CN_NB];         // Ld[j][c] = L[k0 + c][k0 + j]: the diagonal block, a column of L per row
    __shared__ double dv[CN_NB];
    __shared__ int bad;
    const int r = blockIdx.x, tid = threadIdx.x;
    const int R = p.R, Rp = p.Rp;
    const CnRun run = cn_run(p.ws, r, Rp);
    double* A = run.A;
    const double Rd = (double)R;
    if (tid == 0) bad = 0;
    cn_shrink(p, r, run, red);

    if constexpr (!INV) {
        float* out = p.out + (size_t)r * R * R;
        for (int e = tid; e < R * R; e += CN_FT) {
            const int i = e / R, j = e - i * R;
            const double v = A[(size_t)i * Rp + j];
            double o = v;
            if (p.kind == CHEBGCN_CONNECTOME_CORRELATION) {
                const double dd = A[(size_t)i * Rp + i] * A[(size_t)j * Rp + j];
                o = i == j ? 1.0 : dd > 0.0 ? v / sqrt(dd) : 0.0;
            }
            out[e] = (float)o;
        }
        if (tid == 0) {
            p.degenerate[r] = 0;
            run.scal[2] = 0.0;
        }
        return;
    } else {
        const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        const double floor_ = 4.0 * Rd * 0x1p-53;          // a pivot at or below floor_ * Sigma_jj is round-off: the run is degenerate

        // Sigma = L L^T; thread tid = row i.  L[i][p], p < i, replaces A[p][i]; 1 / L[i][i] goes to dinv
        const int i = tid;
        for (int k0 = 0; k0 < R; k0 += CN_NB) {
            cn_acc acc;
#pragma unroll
            for (int j = 0; j < CN_NB; ++j) acc[j] = i < R && i >= k0 && k0 + j < R ? A[(size_t)(k0 + j) * Rp + i] : 0.0;
            for (int p0 = 0; p0 < k0; p0 += CN_PB) {
                cn_stage(A, Rp, p0, k0, k0, Ls);
                __syncthreads();
                if (i < R && i >= k0) {
                    const int n = min(CN_PB, k0 - p0);
#pragma unroll 4
                    for (int pp = 0; pp < n; ++pp) {
                        const double l = A[(size_t)(p0 + pp) * Rp + i];
#pragma unroll
                        for (int j = 0; j < CN_NB; ++j) acc[j] = fma(-l, Ls[pp][j], acc[j]);
                    }
                }
                __syncthreads();
            }
            const int wd = k0 >> 6, base = k0 & 63;
            if (wave == wd) {                       // the diagonal block's rows are 16 lanes of this wave
#pragma unroll 1
                for (int j = 0; j < CN_NB; ++j) {
                    const bool col = k0 + j < R;
                    const double aj = acc[j];
                    const double piv = __shfl(aj, base + j, 64);
                    const double sjj = A[(size_t)min(k0 + j, R - 1) * Rp + min(k0 + j, R - 1)];
                    const bool ok = col && piv > floor_ * sjj && piv < INFINITY;
                    const double d = ok ? sqrt(piv) : 0.0;
                    const double di = ok ? 1.0 / d : 0.0;
                    if (col && !ok) bad = 1;
                    const double l = aj * di;
                    if (lane == base + j) {
                        dv[j] = di;
                        if (col) run.dinv[k0 + j] = di;
                    }
#pragma unroll
                    for (int c = 0; c < CN_NB; ++c) {
                        const double lc = __shfl(l, base + c, 64);          // L[k0 + c][k0 + j]
                        acc[c] = c > j ? fma(-l, lc, acc[c]) : c == j ? l : acc[c];
                    }
                }
                if (lane >= base && lane < base + CN_NB) {
#pragma unroll
                    for (int j = 0; j < CN_NB; ++j) Ld[j][lane - base] = acc[j];
                }
            }
            __syncthreads();
            if (wave > wd) {
#pragma unroll 1
                for (int j = 0; j < CN_NB; ++j) {
                    const double l = acc[j] * dv[j];
#pragma unroll
                    for (int c = 0; c < CN_NB; ++c) acc[c] = c > j ? fma(-l, Ld[j][c], acc[c]) : c == j ? l : acc[c];
                }
            }
            if (i < R) {
#pragma unroll
                for (int j = 0; j < CN_NB; ++j)
                    if (k0 + j < R && i > k0 + j) A[(size_t)(k0 + j) * Rp + i] = acc[j];
            }
            __syncthreads();
        }

        if (tid == 0) {
            p.degenerate[r] = bad;
            run.scal[2] = bad ? 1.0 : 0.0;
        }
    }
}

// workgroup = run: M = L^-1, thread tid = column c; M[i][c], i >= c, replaces A[i][c].  Then the diagonal of P = M^T M
__global__ void __launch_bounds__(CN_FT)
connectome_invert_kernel(double* ws, int R, int Rp) {
    __shared__ double Ls[CN_PB][CN_NB];
    __shared__ double Ld[CN_NB][CN_NB];         // Ld[a][b] = L[i0 + b][i0 + a], a < b
    __shared__ double dv[CN_NB];
    const int r = blockIdx.x, tid = threadIdx.x;
    const CnRun run = cn_run(ws, r, Rp);
    double* A = run.A;
    if (run.scal[2] != 0.0) return;             // degenerate (the same in every thread): the gram kernel writes the identity
    {
        const int c = tid;
        for (int i0 = 0; i0 < R; i0 += CN_NB) {
            cn_acc acc;
#pragma unroll
            for (int q = 0; q < CN_NB; ++q) acc[q] = i0 + q == c ? 1.0 : 0.0;
            if (tid < CN_NB * CN_NB) {
                const int a = tid / CN_NB, b = tid % CN_NB;             // Ld[a][b] = L[i0 + b][i0 + a], a < b
                Ld[a][b] = a < b && i0 + b < R ? A[(size_t)(i0 + a) * Rp + i0 + b] : 0.0;
            }
            if (tid < CN_NB) dv[tid] = i0 + tid < R ? run.dinv[i0 + tid] : 0.0;
            const bool mine = c < R && i0 + CN_NB > c;
            for (int p0 = 0; p0 < i0; p0 += CN_PB) {
                cn_stage(A, Rp, p0, i0, i0, Ls);
                __syncthreads();
                if (mine) {
                    const int n = min(CN_PB, i0 - p0);
#pragma unroll 2
                    for (int pp = max(0, c - p0); pp < n; ++pp) {
                        const double m = A[(size_t)(p0 + pp) * Rp + c];
#pragma unroll
                        for (int q = 0; q < CN_NB; ++q) acc[q] = fma(-Ls[pp][q], m, acc[q]);
                    }
                }
                __syncthreads();
            }
            __syncthreads();
            if (mine) {
#pragma unroll 1
                for (int q = 0; q < CN_NB; ++q) {
                    const double m = acc[q] * dv[q];
#pragma unroll
                    for (int q2 = 0; q2 < CN_NB; ++q2) acc[q2] = q2 > q ? fma(-Ld[q][q2], m, acc[q2]) : q2 == q ? m : acc[q2];
                }
#pragma unroll
                for (int q = 0; q < CN_NB; ++q)
                    if (i0 + q < R && i0 + q >= c) A[(size_t)(i0 + q) * Rp + c] = acc[q];
            }
            __syncthreads();
        }

        // the diagonal of P = M^T M: the chain of the gram kernel's entry (c, c)
        if (c < R) {
            double d = 0.0;
            for (int q = c; q < R; ++q) {
                const double m = A[(size_t)q * Rp + c];
                d = fma(m, m, d);
            }
            run.pdiag[c] = d;
        }
    }
}

// block (tile blockIdx.x, run blockIdx.y): P = M^T M, then the precision or the partial correlation
__global__ void __launch_bounds__(CN_CT)
connectome_gram_kernel(double* __restrict__ ws, int R, int Rp, int kind, float* __restrict__ out) {
    __shared__ double As[CN_TK][CN_TILE], Bs[CN_TK][CN_TILE];
    const int r = blockIdx.y;
    int bi, bj;
    cn_tile_of((int)blockIdx.x, bi, bj);
    const CnRun run = cn_run(ws, r, Rp);
    const double* A = run.A;
    auto load = [&](long long t, int col, double (&v)[4]) {
        const int tr = (int)min(t, (long long)R - 1);
        const int cc = col < Rp ? col : 0;
        const double2 x = *reinterpret_cast<const double2*>(A + (size_t)tr * Rp + cc);
        const double2 y = *reinterpret_cast<const double2*>(A + (size_t)tr * Rp + cc + 2);
        const bool in = t < R;                  // M[t][col + v] lives at and below the diagonal: col + v <= t (< R)
        v[0] = in && col + 0 <= t ? x.x : 0.0;
        v[1] = in && col + 1 <= t ? x.y : 0.0;
        v[2] = in && col + 2 <= t ? y.x : 0.0;
        v[3] = in && col + 3 <= t ? y.y : 0.0;
    };
    const bool degenerate = run.scal[2] != 0.0;     // (the same in every thread)
    double acc[4][4];
    if (!degenerate) cn_tile(acc, (long long)bi * CN_TILE, (long long)R, bi * CN_TILE, bj * CN_TILE, load, As, Bs);
    float* o = out + (size_t)r * R * R;
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gi = bi * CN_TILE + ty * 4 + i, gj = bj * CN_TILE + tx * 4 + j;
            if (gi >= R || gj > gi) continue;
            double v;
            if (degenerate) v = gi == gj ? 1.0 : 0.0;
            else if (kind == CHEBGCN_CONNECTOME_PRECISION) v = acc[i][j];
            else v = gi == gj ? 1.0 : -acc[i][j] / sqrt(run.pdiag[gi] * run.pdiag[gj]);
            const float f = (float)v;
            o[(size_t)gi * R + gj] = f;
            o[(size_t)gj * R + gi] = f;
        }
}

// thread = entry of the mean
__global__ void __launch_bounds__(CN_MT)
connectome_mean_kernel(const float* __restrict__ mats, const int32_t* __restrict__ degenerate, int S, int R, float* __restrict__ mean) {
    const long long e = (long long)blockIdx.x * CN_MT + threadIdx.x;
    const long long n = (long long)R * R;
    if (e >= n) return;
    double s = 0.0;
    int cnt = 0;
    for (int r = 0; r < S; ++r) {
        if (degenerate[r] != 0) continue;
        s = s + (double)mats[(size_t)r * n + e];
        ++cnt;
    }
    mean[e] = cnt ? (float)(s / (double)cnt) : 0.f;
}

static inline bool cn_shape_ok(int S, int R) { return S >= 1 && R >= 1; }
static inline bool cn_served(int S, int R) { return S <= CN_SMAX && R <= CN_RMAX; }
static inline int cn_tiles(int R) {
    const int nb = (R + CN_TILE - 1) / CN_TILE;
    return nb * (nb + 1) / 2;
}

}  // namespace chebgcn

using namespace chebgcn;

extern "C" int chebgcn_connectome_query(int what) {
    switch (what) {
        case 0: return CN_RMAX;             // the largest R
        case 1: return CN_SMAX;             // runs of one call
        case 2: return CN_TILE;             // side of a covariance / gram tile
        case 3: return CN_TK;               // rows of a tile's operands in LDS at once
        case 4: return CN_NB;               // columns of a Cholesky panel
        case 5: return CN_PB;               // finished columns staged in LDS at once
        case 6: return CN_FT;               // threads of a finish workgroup
        case 7: return CN_QW;               // waves (row classes) of the rowsq kernel
        default: return -1;
    }
}

extern "C" size_t chebgcn_connectome_workspace(int S, int R) {
    if (!cn_shape_ok(S, R) || !cn_served(S, R)) return 0;
    return (size_t)S * cn_ws_doubles(plane_stride(R)) * sizeof(double);
}

extern "C" int chebgcn_connectome_cov(const float* series, int64_t Ttot, const int64_t* run_offsets, int S, int R, double* workspace,
                                      size_t workspace_bytes, chebgcn_stream stream_) {
    CG_REQUIRE(series && run_offsets && workspace, "connectome_cov: NULL argument");
    CG_REQUIRE(Ttot >= 1 && cn_shape_ok(S, R), "connectome_cov: bad shape (Ttot = %lld, S = %d, R = %d)", (long long)Ttot, S, R);
    if (!cn_served(S, R) || Ttot > GLM_ELEMS / plane_stride(R))
        return fail(CHEBGCN_EUNSUPPORTED, "connectome_cov: S = %d, R = %d, Ttot = %lld; served: S <= %d, R <= %d, Ttot * Rp <= 2^39", S, R,
                    (long long)Ttot, CN_SMAX, CN_RMAX);
    CG_REQUIRE(workspace_bytes >= chebgcn_connectome_workspace(S, R), "connectome_cov: workspace of %zu bytes, %zu needed", workspace_bytes,
               chebgcn_connectome_workspace(S, R));
    CG_REQUIRE((((uintptr_t)series | (uintptr_t)workspace) & 15) == 0 && ((uintptr_t)run_offsets & 7) == 0,
               "connectome_cov: unaligned argument (16 bytes: a lane loads four regions at once)");
    const int Rp = plane_stride(R);
    hipStream_t stream = (hipStream_t)stream_;
    const long long* offs = (const long long*)run_offsets;
    note_dispatch("connectome_centre_kernel");
    hipLaunchKernelGGL(connectome_centre_kernel, dim3((unsigned)((Rp + CN_MT - 1) / CN_MT), (unsigned)S), dim3(CN_MT), 0, stream, series,
                       (long long)Ttot, offs, R, Rp, workspace);
    note_dispatch_more("connectome_rowsq_kernel");
    hipLaunchKernelGGL(connectome_rowsq_kernel, dim3((unsigned)S), dim3(CN_QW * 64), 0, stream, series, (long long)Ttot, offs, R, Rp,
                       workspace);
    note_dispatch_more("connectome_cov_kernel");
    hipLaunchKernelGGL(connectome_cov_kernel, dim3((unsigned)cn_tiles(R), (unsigned)S), dim3(CN_CT), 0, stream, series, (long long)Ttot,
                       offs, R, Rp, workspace);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_connectome_finish(double* workspace, size_t workspace_bytes, const int64_t* run_offsets, int64_t Ttot, int S, int R,
                                         int kind, double shrinkage, float* matrices, double* shrinkage_out, int32_t* degenerate,
                                         chebgcn_stream stream_) {
    CG_REQUIRE(workspace && run_offsets && matrices && shrinkage_out && degenerate, "connectome_finish: NULL argument");
    CG_REQUIRE(Ttot >= 1 && cn_shape_ok(S, R), "connectome_finish: bad shape (Ttot = %lld, S = %d, R = %d)", (long long)Ttot, S, R);
    CG_REQUIRE(kind >= CHEBGCN_CONNECTOME_COVARIANCE && kind <= CHEBGCN_CONNECTOME_PARTIAL, "connectome_finish: unknown kind %d", kind);
    CG_REQUIRE(shrinkage < 0.0 || shrinkage <= 1.0, "connectome_finish: a shrinkage of %g is neither negative (Ledoit-Wolf) nor in [0, 1]",
               shrinkage);
    if (!cn_served(S, R))
        return fail(CHEBGCN_EUNSUPPORTED, "connectome_finish: S = %d, R = %d; served: S <= %d, R <= %d", S, R, CN_SMAX, CN_RMAX);
    CG_REQUIRE(workspace_bytes >= chebgcn_connectome_workspace(S, R), "connectome_finish: workspace of %zu bytes, %zu needed",
               workspace_bytes, chebgcn_connectome_workspace(S, R));
    CG_REQUIRE(((uintptr_t)workspace & 15) == 0 && (((uintptr_t)run_offsets | (uintptr_t)shrinkage_out) & 7) == 0 &&
                   (((uintptr_t)matrices | (uintptr_t)degenerate) & 3) == 0,
               "connectome_finish: unaligned argument");
    const int Rp = plane_stride(R);
    hipStream_t stream = (hipStream_t)stream_;
    CnFinish p{workspace, (const long long*)run_offsets, (long long)Ttot, R, Rp, kind, shrinkage < 0.0 ? -1.0 : shrinkage, matrices,
               shrinkage_out, degenerate};
    if (kind <= CHEBGCN_CONNECTOME_CORRELATION) {
        note_dispatch("connectome_finish_kernel<plain>");
        hipLaunchKernelGGL(connectome_finish_kernel<false>, dim3((unsigned)S), dim3(CN_FT), 0, stream, p);
    } else {
        note_dispatch("connectome_finish_kernel<inverse>");
        hipLaunchKernelGGL(connectome_finish_kernel<true>, dim3((unsigned)S), dim3(CN_FT), 0, stream, p);
        note_dispatch_more("connectome_invert_kernel");
        hipLaunchKernelGGL(connectome_invert_kernel, dim3((unsigned)S), dim3(CN_FT), 0, stream, workspace, R, Rp);
        note_dispatch_more("connectome_gram_kernel");
        hipLaunchKernelGGL(connectome_gram_kernel, dim3((unsigned)cn_tiles(R), (unsigned)S), dim3(CN_CT), 0, stream, workspace, R, Rp, kind,
                           matrices);
    }
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_connectome_sigma(double* workspace, size_t workspace_bytes, const int64_t* run_offsets, int64_t Ttot, int S, int R,
                                        double shrinkage, double* sigma, double* shrinkage_out, chebgcn_stream stream_) {
    CG_REQUIRE(workspace && run_offsets && sigma && shrinkage_out, "connectome_sigma: NULL argument");
    CG_REQUIRE(Ttot >= 1 && cn_shape_ok(S, R), "connectome_sigma: bad shape (Ttot = %lld, S = %d, R = %d)", (long long)Ttot, S, R);
    CG_REQUIRE(shrinkage < 0.0 || shrinkage <= 1.0, "connectome_sigma: a shrinkage of %g is neither negative (Ledoit-Wolf) nor in [0, 1]",
               shrinkage);
    if (!cn_served(S, R))
        return fail(CHEBGCN_EUNSUPPORTED, "connectome_sigma: S = %d, R = %d; served: S <= %d, R <= %d", S, R, CN_SMAX, CN_RMAX);
    CG_REQUIRE(workspace_bytes >= chebgcn_connectome_workspace(S, R), "connectome_sigma: workspace of %zu bytes, %zu needed",
               workspace_bytes, chebgcn_connectome_workspace(S, R));
    CG_REQUIRE(((uintptr_t)workspace & 15) == 0 && (((uintptr_t)run_offsets | (uintptr_t)shrinkage_out | (uintptr_t)sigma) & 7) == 0,
               "connectome_sigma: unaligned argument");
    CnFinish p{workspace, (const long long*)run_offsets, (long long)Ttot, R, plane_stride(R), CHEBGCN_CONNECTOME_COVARIANCE,
               shrinkage < 0.0 ? -1.0 : shrinkage, nullptr, shrinkage_out, nullptr};
    note_dispatch("connectome_sigma_kernel");
    hipLaunchKernelGGL(connectome_sigma_kernel, dim3((unsigned)S), dim3(CN_FT), 0, (hipStream_t)stream_, p, sigma);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_connectome_mean(const float* matrices, const int32_t* degenerate, int S, int R, float* mean, chebgcn_stream stream_) {
    CG_REQUIRE(matrices && degenerate && mean, "connectome_mean: NULL argument");
    CG_REQUIRE(cn_shape_ok(S, R), "connectome_mean: bad shape (S = %d, R = %d)", S, R);
    if (S > (1 << 24) || R > CN_RMAX)
        return fail(CHEBGCN_EUNSUPPORTED, "connectome_mean: S = %d, R = %d; served: S <= 2^24, R <= %d", S, R, CN_RMAX);
    CG_REQUIRE((((uintptr_t)matrices | (uintptr_t)degenerate | (uintptr_t)mean) & 3) == 0, "connectome_mean: unaligned argument");
    note_dispatch("connectome_mean_kernel");
    hipLaunchKernelGGL(connectome_mean_kernel, dim3((unsigned)((R * R + CN_MT - 1) / CN_MT)), dim3(CN_MT), 0, (hipStream_t)stream_, matrices,
                       degenerate, S, R, mean);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}
