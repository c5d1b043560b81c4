// Tangent-space connectivity (connectome.tangent): a batched float64 symmetric eigensolver for R <= 512 and the products around
// it -- a matrix function V f(a Lambda) V^T, the congruence W A W, the mean of the unflagged matrices and its Frobenius norm.
// include/chebgcn.h states the arithmetic and the order of every sum; DESIGN 4.34 tells why each choice.
//
// The solver is a block Jacobi method on X = A V and V, both kept TRANSPOSED (row p of Xt / Vt is column p: contiguous), columns
// cut into blocks of TG_B = 8, block pairs in round-robin order, one launch per step, workgroup = (block pair, matrix):
//
//   tangent_eigh_init_kernel    workgroup = matrix: Xt <- A, Vt <- I, the rotation floor R 2^-53 max|a_ij|, the counters.
//   tangent_eigh_step_kernel    256 threads.  The pair's 16 columns of X and of V go to LDS (column stride R | 1: sixteen columns
//                               on sixteen banks).  Thread (i, j) forms T_ij = (v_i . x_j + v_j . x_i) / 2, each dot ONE chain over
//                               ascending rows, the pair (i, j) and (j, i) from the same two chains: T = sym(V_blk^T A V_blk) is
//                               symmetric bit for bit.  A two-sided Jacobi on T (16 x 16) in the round-robin order of its own,
//                               eight disjoint rotations at a time, accumulates Q; then X_blk <- X_blk Q, V_blk <- V_blk Q, every
//                               entry one chain over ascending columns of the pair.  A workgroup that rotated nothing writes nothing.
//   tangent_eigh_sweep_kernel   one workgroup: a matrix whose sweep rotated nothing is done; counts the matrices still open.
//   tangent_eigh_values_kernel  thread (p, matrix): lambda_p = v_p . x_p, the Rayleigh quotient (signed), one chain.
//   tangent_fvals_kernel        thread (p, matrix): f(a lambda_p); a lambda the function cannot take flags the matrix.
//   tangent_product_kernel<lower|full>  C_ij = sum_p a_pi b_pj on 64 x 64 tiles, 256 threads, 4 x 4 accumulators a thread, 16 rows
//                               of the operands in LDS at a time (the tile shape of connectome_cov_kernel); ONE chain over ascending
//                               p; <lower> forms the lower triangle and mirrors it.
//   tangent_mean_kernel         thread = entry: the chain acc + m_s over the unflagged matrices in ascending s.
//   tangent_norm_kernel         one workgroup of 512: the Frobenius norm by chains and a fixed tree.
// Rotations are counted with integer atomics; no float atomics anywhere.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace chebgcn {

constexpr int TG_RMAX = 512;
constexpr int TG_SMAX = 65535;              // matrices of one call (grid.y)
constexpr int TG_B = 8;                     // columns of a block
constexpr int TG_P = 2 * TG_B;              // columns of a block pair
constexpr int TG_T = 256;                   // threads of a step workgroup: one per entry of T
constexpr int TG_SWEEPS = 40;               // sweeps before a matrix is reported as not converged
constexpr int TG_INNER = 10;                // sweeps of the Jacobi on T; what they leave the next outer sweep takes up
constexpr int TG_TILE = 64;                 // a product tile is TG_TILE x TG_TILE
constexpr int TG_TK = 16;                   // rows of a tile's operands in LDS at once
constexpr int TG_NT = 512;                  // threads of the norm workgroup
constexpr int TG_LD = TG_P + 1;             // row stride of T and Q in LDS

// the workspace of chebgcn_sym_eigh for S matrices: Xt [S][R][R], the floors [S], then int32 {rot [S], done [S], sweeps [S], open}
__host__ __device__ constexpr size_t tg_ws_bytes(int S, int R) {
    return ((size_t)S * R * R + (size_t)S) * sizeof(double) + ((size_t)3 * S + 2) * sizeof(int32_t);
}
struct TgWs {
    double* Xt;
    double* floor_;
    int32_t* rot;
    int32_t* done;
    int32_t* sweeps;
    int32_t* open;
};
__host__ __device__ inline TgWs tg_ws(void* ws, int S, int R) {
    double* x = (double*)ws;
    double* f = x + (size_t)S * R * R;
    int32_t* i = (int32_t*)(f + S);
    return TgWs{x, f, i, i + S, i + 2 * S, i + 3 * S};
}

// blocks (a, b) of pair k at step st of the round robin over m (even) players: player m - 1 stays, the others turn
__device__ __forceinline__ void tg_pair(int m, int st, int k, int& a, int& b) {
    if (k == 0) {
        a = st;
        b = m - 1;
    } else {
        a = (st + k) % (m - 1);
        b = (st - k + (m - 1)) % (m - 1);
    }
    if (a > b) {
        const int t = a;
        a = b;
        b = t;
    }
}

// workgroup = matrix
__global__ void __launch_bounds__(TG_T)
tangent_eigh_init_kernel(const double* __restrict__ A, int S, int R, double* __restrict__ Vt, void* ws_) {
    __shared__ double red[TG_T];
    const int s = blockIdx.x, tid = threadIdx.x;
    const TgWs ws = tg_ws(ws_, S, R);
    const size_t n = (size_t)R * R;
    const double* a = A + (size_t)s * n;
    double* x = ws.Xt + (size_t)s * n;
    double* v = Vt + (size_t)s * n;
    double m = 0.0;
    for (size_t e = tid; e < n; e += TG_T) {
        const double val = a[e];
        x[e] = val;
        v[e] = e / R == e % R ? 1.0 : 0.0;
        m = fmax(m, fabs(val));                 // (a NaN entry does not raise the floor; it stops the rotations it meets)
    }
    red[tid] = m;
    __syncthreads();
    for (int h = TG_T / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] = fmax(red[tid], red[tid + h]);
        __syncthreads();
    }
    if (tid == 0) {
        ws.floor_[s] = ((double)R * 0x1p-53) * red[0];
        ws.rot[s] = 0;
        ws.done[s] = 0;
        ws.sweeps[s] = 0;
    }
}

// block (pair blockIdx.x, matrix blockIdx.y)
__global__ void __launch_bounds__(TG_T)
tangent_eigh_step_kernel(int S, int R, int nb, int m, int st, double* __restrict__ Vt, void* ws_) {
    extern __shared__ __attribute__((aligned(16))) double tg_cols[];       // Xs [TG_P][ldc], then Vs [TG_P][ldc]
    __shared__ double Ts[2][TG_P][TG_LD], Qs[2][TG_P][TG_LD];
    __shared__ double cs[TG_P], sn[TG_P];       // per index: c, and s signed for its side of the pair
    __shared__ int partner[TG_P];
    __shared__ int nrot, nstep;
    const int s = blockIdx.y, tid = threadIdx.x;
    const TgWs ws = tg_ws(ws_, S, R);
    if (ws.done[s] != 0) return;                // (the same in every thread)
    int ba, bb;
    tg_pair(m, st, (int)blockIdx.x, ba, bb);
    if (bb >= nb && nb > 1) return;             // the bye of an odd block count; a matrix of one block works on that block alone
    const int ldc = R | 1;
    double* Xs = tg_cols;
    double* Vs = tg_cols + (size_t)TG_P * ldc;
    const size_t n = (size_t)R * R;
    double* xg = ws.Xt + (size_t)s * n;
    double* vg = Vt + (size_t)s * n;
    // column c of the pair = column col(c) of the matrix, or none (beyond R, or the absent second block)
    auto col_of = [&](int c) {
        const int col = (c < TG_B ? ba : bb) * TG_B + (c & (TG_B - 1));
        return (c < TG_B || bb < nb) && col < R ? col : -1;
    };
#pragma unroll 1
    for (int c = 0; c < TG_P; ++c) {
        const int col = col_of(c);
        for (int r = tid; r < R; r += TG_T) {
            Xs[c * ldc + r] = col >= 0 ? xg[(size_t)col * R + r] : 0.0;
            Vs[c * ldc + r] = col >= 0 ? vg[(size_t)col * R + r] : 0.0;
        }
    }
    if (tid == 0) nrot = 0;
    __syncthreads();

    // T = sym(V^T X): thread (i, j) and thread (j, i) run the same two chains
    const int i = tid >> 4, j = tid & 15;
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    {
        const double* vl = Vs + lo * ldc;
        const double* vh = Vs + hi * ldc;
        const double* xl = Xs + lo * ldc;
        const double* xh = Xs + hi * ldc;
        double t1 = 0.0, t2 = 0.0;
#pragma unroll 4
        for (int r = 0; r < R; ++r) {
            t1 = fma(vl[r], xh[r], t1);
            t2 = fma(vh[r], xl[r], t2);
        }
        Ts[0][i][j] = 0.5 * (t1 + t2);
        Qs[0][i][j] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();

    const double tau = (double)R * 0x1p-53, floor_ = ws.floor_[s];
    int cur = 0;
    for (int sweep = 0; sweep < TG_INNER; ++sweep) {
        if (tid == 0) nstep = 0;
        for (int u = 0; u < TG_P - 1; ++u) {
            if (tid < TG_B) {
                int p, q;
                tg_pair(TG_P, u, tid, p, q);
                const double g = Ts[cur][p][q], app = Ts[cur][p][p], aqq = Ts[cur][q][q];
                const double thr = fmax(tau * sqrt(fabs(app * aqq)), floor_);
                double c = 1.0, sgn = 0.0;
                if (fabs(g) > thr && fabs(g) < INFINITY) {         // (false for a NaN)
                    const double zeta = (aqq - app) / (2.0 * g);
                    const double az = fabs(zeta);
                    const double t = az > 0x1p500 ? 0.5 / zeta : (zeta >= 0.0 ? 1.0 : -1.0) / (az + sqrt(fma(zeta, zeta, 1.0)));
                    c = 1.0 / sqrt(fma(t, t, 1.0));
                    sgn = c * t;
                    atomicAdd(&nstep, 1);
                }
                cs[p] = c;
                cs[q] = c;
                sn[p] = -sgn;               // new column p = c col p - s col q
                sn[q] = sgn;                // new column q = s col p + c col q
                partner[p] = q;
                partner[q] = p;
            }
            __syncthreads();
            {
                // T' = J^T T J on the entry (lo, hi), the same arithmetic in both of its threads; Q' = Q J
                const int pl = partner[lo], ph = partner[hi];
                const double cl = cs[lo], sl = sn[lo], ch = cs[hi], sh = sn[hi];
                double tn;
                if (sl == 0.0 && sh == 0.0) {
                    tn = Ts[cur][lo][hi];
                } else if (pl == hi) {
                    tn = 0.0;                   // the entry the rotation annihilates
                } else {
                    const double a0 = fma(sh, Ts[cur][lo][ph], ch * Ts[cur][lo][hi]);
                    const double a1 = fma(sh, Ts[cur][pl][ph], ch * Ts[cur][pl][hi]);
                    tn = fma(sl, a1, cl * a0);
                }
                Ts[cur ^ 1][i][j] = tn;
                const int pj = partner[j];
                const double cj = cs[j], sj = sn[j];
                Qs[cur ^ 1][i][j] = sj == 0.0 ? Qs[cur][i][j] : fma(sj, Qs[cur][i][pj], cj * Qs[cur][i][j]);
            }
            cur ^= 1;
            __syncthreads();
        }
        const int made = nstep;
        __syncthreads();
        if (tid == 0) nrot += made;
        if (made == 0) break;                   // (the same in every thread)
    }
    __syncthreads();
    if (nrot == 0) return;                      // Q is the identity: nothing to write
    if (tid == 0) atomicAdd(&ws.rot[s], nrot);

    // X_blk <- X_blk Q, V_blk <- V_blk Q; thread = row
    int cols[TG_P];
#pragma unroll
    for (int c = 0; c < TG_P; ++c) cols[c] = col_of(c);
    // (rows tid and tid + TG_T of X and of V at once: every entry of Q is read once and none is kept)
    const int r0 = tid, r1 = tid + TG_T;
    const int l0 = r0 < R ? r0 : 0, l1 = r1 < R ? r1 : 0;
    double ax0[TG_P], ax1[TG_P], av0[TG_P], av1[TG_P];
#pragma unroll
    for (int d = 0; d < TG_P; ++d) ax0[d] = ax1[d] = av0[d] = av1[d] = 0.0;
#pragma unroll 1                                // (unrolled, the compiler reads all of Q ahead and spills: 580 bytes of scratch a lane)
    for (int c = 0; c < TG_P; ++c) {
        const double x0 = Xs[c * ldc + l0], x1 = Xs[c * ldc + l1], v0 = Vs[c * ldc + l0], v1 = Vs[c * ldc + l1];
#pragma unroll
        for (int d = 0; d < TG_P; ++d) {
            const double qv = Qs[cur][c][d];
            ax0[d] = fma(x0, qv, ax0[d]);
            ax1[d] = fma(x1, qv, ax1[d]);
            av0[d] = fma(v0, qv, av0[d]);
            av1[d] = fma(v1, qv, av1[d]);
        }
    }
#pragma unroll
    for (int d = 0; d < TG_P; ++d) {
        if (cols[d] < 0) continue;
        if (r0 < R) {
            xg[(size_t)cols[d] * R + r0] = ax0[d];
            vg[(size_t)cols[d] * R + r0] = av0[d];
        }
        if (r1 < R) {
            xg[(size_t)cols[d] * R + r1] = ax1[d];
            vg[(size_t)cols[d] * R + r1] = av1[d];
        }
    }
}
static_assert(TG_RMAX <= 2 * TG_T, "a thread of the step kernel owns two rows");

// one workgroup
__global__ void __launch_bounds__(TG_T)
tangent_eigh_sweep_kernel(int S, int R, void* ws_) {
    __shared__ int open;
    const TgWs ws = tg_ws(ws_, S, R);
    if (threadIdx.x == 0) open = 0;
    __syncthreads();
    int mine = 0;
    for (int s = threadIdx.x; s < S; s += TG_T) {
        if (ws.done[s] == 0) {
            ws.sweeps[s] += 1;
            if (ws.rot[s] == 0) ws.done[s] = 1;
            ws.rot[s] = 0;
        }
        mine += ws.done[s] == 0;
    }
    if (mine) atomicAdd(&open, mine);
    __syncthreads();
    if (threadIdx.x == 0) *ws.open = open;
}

// thread (p, matrix blockIdx.y)
__global__ void __launch_bounds__(TG_T)
tangent_eigh_values_kernel(int S, int R, const double* __restrict__ Vt, void* ws_, double* __restrict__ w, int32_t* __restrict__ sweeps,
                           int32_t* __restrict__ converged) {
    const int p = blockIdx.x * TG_T + threadIdx.x, s = blockIdx.y;
    const TgWs ws = tg_ws(ws_, S, R);
    if (p >= R) return;
    const double* x = ws.Xt + ((size_t)s * R + p) * R;
    const double* v = Vt + ((size_t)s * R + p) * R;
    double acc = 0.0;
#pragma unroll 4
    for (int r = 0; r < R; ++r) acc = fma(v[r], x[r], acc);
    w[(size_t)s * R + p] = acc;
    if (p == 0) {
        sweeps[s] = ws.sweeps[s];
        converged[s] = ws.done[s];
    }
}

// thread (p, matrix blockIdx.y)
__global__ void __launch_bounds__(TG_T)
tangent_fvals_kernel(const double* __restrict__ w, int R, int func, double a, double* __restrict__ fvals, int32_t* __restrict__ flags) {
    const int p = blockIdx.x * TG_T + threadIdx.x, s = blockIdx.y;
    if (p >= R) return;
    const double x = a * w[(size_t)s * R + p];
    const bool finite = fabs(x) < INFINITY;
    double f;
    bool ok;
    switch (func) {
        case CHEBGCN_SYM_LOG: ok = finite && x > 0.0; f = ok ? log(x) : 0.0; break;
        case CHEBGCN_SYM_EXP: f = exp(x); ok = finite && f < INFINITY; break;
        case CHEBGCN_SYM_SQRT: ok = finite && x > 0.0; f = ok ? sqrt(x) : 0.0; break;
        default: ok = finite && x > 0.0; f = ok ? 1.0 / sqrt(x) : 0.0; break;
    }
    fvals[(size_t)s * R + p] = ok ? f : 0.0;
    if (!ok) flags[s] = 1;                      // (every thread that stores, stores 1)
}

// tile x of the lower triangle, row-major: (bi, bj), bj <= bi
__device__ __forceinline__ void tg_tile_of(int x, int& bi, int& bj) {
    bi = 0;
    while ((bi + 1) * (bi + 2) / 2 <= x) ++bi;
    bj = x - bi * (bi + 1) / 2;
}

struct TgProduct {
    const double* a;            // [R][R], matrix s at a + s * a_stride; the entry (p, i) scaled by scale[s][p] where scale is given
    const double* b;
    size_t a_stride, b_stride;
    const double* scale;        // [S][R] or NULL
    const int32_t* flags;       // [S] or NULL: a flagged matrix comes out as zeros
    double* out64;              // [S][R][R], or
    float* out32;
    int R;
};

// block (tile blockIdx.x, matrix blockIdx.y): C_ij = sum_p a_pi b_pj
template <bool LOWER>
__global__ void __launch_bounds__(TG_T)
tangent_product_kernel(TgProduct q) {
    __shared__ double As[TG_TK][TG_TILE], Bs[TG_TK][TG_TILE];
    const int s = blockIdx.y, R = q.R, tid = threadIdx.x;
    int bi, bj;
    if (LOWER) {
        tg_tile_of((int)blockIdx.x, bi, bj);
    } else {
        const int nbt = (R + TG_TILE - 1) / TG_TILE;
        bi = (int)blockIdx.x / nbt;
        bj = (int)blockIdx.x % nbt;
    }
    const double* a = q.a + (size_t)s * q.a_stride;
    const double* b = q.b + (size_t)s * q.b_stride;
    const double* sc = q.scale ? q.scale + (size_t)s * R : nullptr;
    const bool flagged = q.flags && q.flags[s] != 0;        // (the same in every thread)
    const int lr = tid >> 4, lc = (tid & 15) * 4, ty = tid >> 4, tx = tid & 15;
    double acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
    if (!flagged) {
        for (int p0 = 0; p0 < R; p0 += TG_TK) {
            const int p = p0 + lr;
            const double f = p < R ? (sc ? sc[p] : 1.0) : 0.0;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int ca = bi * TG_TILE + lc + v, cb = bj * TG_TILE + lc + v;
                As[lr][lc + v] = p < R && ca < R ? f * a[(size_t)p * R + ca] : 0.0;
                Bs[lr][lc + v] = p < R && cb < R ? b[(size_t)p * R + cb] : 0.0;
            }
            __syncthreads();
#pragma unroll 4
            for (int k = 0; k < TG_TK; ++k) {
                double av[4], bv[4];
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    av[v] = As[k][ty * 4 + v];
                    bv[v] = Bs[k][tx * 4 + v];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) acc[u][v] = fma(av[u], bv[v], acc[u][v]);
            }
            __syncthreads();
        }
    }
    const size_t n = (size_t)R * R;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int gi = bi * TG_TILE + ty * 4 + u, gj = bj * TG_TILE + tx * 4 + v;
            if (gi >= R || gj >= R || (LOWER && gj > gi)) continue;
            const double val = acc[u][v];
            if (q.out64) {
                q.out64[s * n + (size_t)gi * R + gj] = val;
                if (LOWER) q.out64[s * n + (size_t)gj * R + gi] = val;
            } else {
                q.out32[s * n + (size_t)gi * R + gj] = (float)val;
                if (LOWER) q.out32[s * n + (size_t)gj * R + gi] = (float)val;
            }
        }
}

// thread = entry
__global__ void __launch_bounds__(TG_T)
tangent_mean_kernel(const double* __restrict__ mats, const int32_t* __restrict__ flags, int S, int R, int first, int n_total,
                    double* __restrict__ acc, double* __restrict__ mean) {
    const long long e = (long long)blockIdx.x * TG_T + threadIdx.x;
    const long long n = (long long)R * R;
    if (e >= n) return;
    double a = first ? 0.0 : acc[e];
    for (int s = 0; s < S; ++s) {
        if (flags[s] != 0) continue;
        a = a + mats[(size_t)s * n + e];
    }
    acc[e] = a;
    if (n_total > 0) mean[e] = a / (double)n_total;
}

// one workgroup
__global__ void __launch_bounds__(TG_NT)
tangent_norm_kernel(const double* __restrict__ mean, int R, double* __restrict__ norm) {
    __shared__ double red[TG_NT];
    const int tid = threadIdx.x;
    double part = 0.0;
    for (int e = tid; e < R * R; e += TG_NT) part = fma(mean[e], mean[e], part);
    red[tid] = part;
    __syncthreads();
    for (int h = TG_NT / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] = red[tid] + red[tid + h];
        __syncthreads();
    }
    if (tid == 0) norm[0] = sqrt(red[0]);
}

static inline bool tg_shape_ok(int S, int R) { return S >= 1 && R >= 1; }
static inline bool tg_served(int S, int R) { return S <= TG_SMAX && R <= TG_RMAX; }
static inline bool tg_aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }
static inline bool tg_aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }
static inline int tg_tiles_lower(int R) {
    const int nb = (R + TG_TILE - 1) / TG_TILE;
    return nb * (nb + 1) / 2;
}
static inline int tg_tiles_full(int R) {
    const int nb = (R + TG_TILE - 1) / TG_TILE;
    return nb * nb;
}

}  // namespace chebgcn

using namespace chebgcn;

extern "C" int chebgcn_tangent_query(int what) {
    switch (what) {
        case 0: return TG_RMAX;             // the largest R
        case 1: return TG_SMAX;             // matrices of one call
        case 2: return TG_B;                // columns of a Jacobi block
        case 3: return TG_T;                // threads of a step workgroup: a thread's second row starts here
        case 4: return TG_SWEEPS;           // the cap of sweeps
        case 5: return TG_TILE;             // side of a product tile
        case 6: return TG_TK;               // rows of a tile's operands in LDS at once
        case 7: return TG_INNER;            // sweeps of the Jacobi inside a block pair
        default: return -1;
    }
}

extern "C" size_t chebgcn_tangent_workspace(int S, int R) {
    if (!tg_shape_ok(S, R) || !tg_served(S, R)) return 0;
    return tg_ws_bytes(S, R);
}

extern "C" int chebgcn_sym_eigh(const double* A, int S, int R, double* w, double* Vt, int32_t* sweeps, int32_t* converged, void* workspace,
                                size_t workspace_bytes, chebgcn_stream stream_) {
    CG_REQUIRE(A && w && Vt && sweeps && converged && workspace, "sym_eigh: NULL argument");
    CG_REQUIRE(tg_shape_ok(S, R), "sym_eigh: bad shape (S = %d, R = %d)", S, R);
    if (!tg_served(S, R)) return fail(CHEBGCN_EUNSUPPORTED, "sym_eigh: S = %d, R = %d; served: S <= %d, R <= %d", S, R, TG_SMAX, TG_RMAX);
    CG_REQUIRE(workspace_bytes >= tg_ws_bytes(S, R), "sym_eigh: workspace of %zu bytes, %zu needed", workspace_bytes, tg_ws_bytes(S, R));
    CG_REQUIRE(tg_aligned8(A) && tg_aligned8(w) && tg_aligned8(Vt) && tg_aligned8(workspace) && tg_aligned4(sweeps) && tg_aligned4(converged),
               "sym_eigh: unaligned argument");
    CG_REQUIRE((const void*)A != (const void*)Vt, "sym_eigh: Vt must not alias A");
    hipStream_t stream = (hipStream_t)stream_;
    const int nb = (R + TG_B - 1) / TG_B;
    const int m = nb + (nb & 1);                // players of the round robin: an odd count plays with one bye
    const size_t lds = (size_t)2 * TG_P * (R | 1) * sizeof(double);
    if (lds > 48 * 1024)                        // (an attribute of the function on the current device; no allocation)
        CG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(tangent_eigh_step_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
    const TgWs ws = tg_ws(workspace, S, R);
    note_dispatch("tangent_eigh_init_kernel");
    hipLaunchKernelGGL(tangent_eigh_init_kernel, dim3((unsigned)S), dim3(TG_T), 0, stream, A, S, R, Vt, workspace);
    note_dispatch_more("tangent_eigh_step_kernel");
    note_dispatch_more("tangent_eigh_sweep_kernel");
    for (int sweep = 0; sweep < TG_SWEEPS; ++sweep) {
        for (int st = 0; st < m - 1; ++st)
            hipLaunchKernelGGL(tangent_eigh_step_kernel, dim3((unsigned)(m / 2), (unsigned)S), dim3(TG_T), lds, stream, S, R, nb, m, st, Vt,
                               workspace);
        hipLaunchKernelGGL(tangent_eigh_sweep_kernel, dim3(1), dim3(TG_T), 0, stream, S, R, workspace);
        CG_HIP(hipGetLastError());
        int32_t open = 0;                       // the one readback of a sweep: matrices still rotating
        CG_HIP(hipMemcpyAsync(&open, ws.open, sizeof(open), hipMemcpyDeviceToHost, stream));
        CG_HIP(hipStreamSynchronize(stream));
        if (open == 0) break;
    }
    note_dispatch_more("tangent_eigh_values_kernel");
    hipLaunchKernelGGL(tangent_eigh_values_kernel, dim3((unsigned)((R + TG_T - 1) / TG_T), (unsigned)S), dim3(TG_T), 0, stream, S, R, Vt,
                       workspace, w, sweeps, converged);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_sym_function(const double* w, const double* Vt, int S, int R, int func, double a, void* out, int out_float32,
                                    int32_t* flags, double* fvals, chebgcn_stream stream_) {
    CG_REQUIRE(w && Vt && out && flags && fvals, "sym_function: NULL argument");
    CG_REQUIRE(tg_shape_ok(S, R), "sym_function: bad shape (S = %d, R = %d)", S, R);
    CG_REQUIRE(func >= CHEBGCN_SYM_LOG && func <= CHEBGCN_SYM_RSQRT, "sym_function: unknown function %d", func);
    CG_REQUIRE(fabs(a) < INFINITY, "sym_function: a = %g is not finite", a);
    CG_REQUIRE(out_float32 == 0 || out_float32 == 1, "sym_function: out_float32 must be 0 or 1, got %d", out_float32);
    if (!tg_served(S, R))
        return fail(CHEBGCN_EUNSUPPORTED, "sym_function: S = %d, R = %d; served: S <= %d, R <= %d", S, R, TG_SMAX, TG_RMAX);
    CG_REQUIRE(tg_aligned8(w) && tg_aligned8(Vt) && tg_aligned8(fvals) && tg_aligned4(flags) &&
                   (out_float32 ? tg_aligned4(out) : tg_aligned8(out)), "sym_function: unaligned argument");
    hipStream_t stream = (hipStream_t)stream_;
    note_dispatch("tangent_fvals_kernel");
    hipLaunchKernelGGL(tangent_fvals_kernel, dim3((unsigned)((R + TG_T - 1) / TG_T), (unsigned)S), dim3(TG_T), 0, stream, w, R, func, a, fvals,
                       flags);
    const size_t n = (size_t)R * R;
    TgProduct q{Vt, Vt, n, n, fvals, flags, out_float32 ? nullptr : (double*)out, out_float32 ? (float*)out : nullptr, R};
    note_dispatch_more("tangent_product_kernel<lower>");
    hipLaunchKernelGGL(tangent_product_kernel<true>, dim3((unsigned)tg_tiles_lower(R), (unsigned)S), dim3(TG_T), 0, stream, q);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_sym_congruence(const double* W, const double* A, int S, int R, double* out, double* scratch, chebgcn_stream stream_) {
    CG_REQUIRE(W && A && out && scratch, "sym_congruence: NULL argument");
    CG_REQUIRE(tg_shape_ok(S, R), "sym_congruence: bad shape (S = %d, R = %d)", S, R);
    if (!tg_served(S, R))
        return fail(CHEBGCN_EUNSUPPORTED, "sym_congruence: S = %d, R = %d; served: S <= %d, R <= %d", S, R, TG_SMAX, TG_RMAX);
    CG_REQUIRE(tg_aligned8(W) && tg_aligned8(A) && tg_aligned8(out) && tg_aligned8(scratch), "sym_congruence: unaligned argument");
    CG_REQUIRE(scratch != out && scratch != A && scratch != W, "sym_congruence: scratch must not alias an operand");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t n = (size_t)R * R;
    // scratch_s = A_s W (A symmetric: a_pi = A[p][i]); out_s = W scratch_s (W symmetric), the lower triangle mirrored
    TgProduct q1{A, W, n, 0, nullptr, nullptr, scratch, nullptr, R};
    note_dispatch("tangent_product_kernel<full>");
    hipLaunchKernelGGL(tangent_product_kernel<false>, dim3((unsigned)tg_tiles_full(R), (unsigned)S), dim3(TG_T), 0, stream, q1);
    TgProduct q2{W, scratch, 0, n, nullptr, nullptr, out, nullptr, R};
    note_dispatch_more("tangent_product_kernel<lower>");
    hipLaunchKernelGGL(tangent_product_kernel<true>, dim3((unsigned)tg_tiles_lower(R), (unsigned)S), dim3(TG_T), 0, stream, q2);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_sym_mean(const double* matrices, const int32_t* flags, int S, int R, int first, int n_total, double* acc, double* mean,
                                double* norm, chebgcn_stream stream_) {
    CG_REQUIRE(matrices && flags && acc, "sym_mean: NULL argument");
    CG_REQUIRE(tg_shape_ok(S, R), "sym_mean: bad shape (S = %d, R = %d)", S, R);
    CG_REQUIRE(n_total >= 0 && (first == 0 || first == 1), "sym_mean: first = %d, n_total = %d", first, n_total);
    CG_REQUIRE(n_total == 0 || (mean && norm), "sym_mean: the last pass needs mean and norm");
    if (S > (1 << 24) || R > TG_RMAX) return fail(CHEBGCN_EUNSUPPORTED, "sym_mean: S = %d, R = %d; served: S <= 2^24, R <= %d", S, R, TG_RMAX);
    CG_REQUIRE(tg_aligned8(matrices) && tg_aligned4(flags) && tg_aligned8(acc) && tg_aligned8(mean) && tg_aligned8(norm),
               "sym_mean: unaligned argument");
    hipStream_t stream = (hipStream_t)stream_;
    note_dispatch("tangent_mean_kernel");
    hipLaunchKernelGGL(tangent_mean_kernel, dim3((unsigned)((R * R + TG_T - 1) / TG_T)), dim3(TG_T), 0, stream, matrices, flags, S, R, first,
                       n_total, acc, mean);
    if (n_total > 0) {
        note_dispatch_more("tangent_norm_kernel");
        hipLaunchKernelGGL(tangent_norm_kernel, dim3(1), dim3(TG_NT), 0, stream, (const double*)mean, R, norm);
    }
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}
