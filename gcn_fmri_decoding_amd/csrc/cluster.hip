// Permutation inference on maps (stats.map_test, stats.design_test): t maps of permutations and their cluster enhancement on the
// brain graph.
//
//   signflip_t       t[p][v] of permutation p0 + p from x [S][M]: float64 on the vector ALU, every operation rounded on its own
//                    (include/chebgcn.h states them one by one), one thread per (permutation, vertex), the S signs of the
//                    permutation in LDS (drawn from chebgcn_aug_draw or unpacked from the caller's table).
//   perm_glm_t       t[p][v] of one contrast of a group design whose rows permutation p permutes (stats.design_test): described
//                    where it stands, below signflip_t.
//   cluster_enhance  per permutation: u = +-t, the heights i = n .. 1 walked DOWNWARDS (hf[i] falls, so components only merge and
//                    the forest of height i + 1 seeds height i), at every height the connected components of {v : u[v] > hf[i]},
//                    their sizes, and acc[v] = acc[v] + ep[size] * hw[i] for the active vertices.
//
// A vertex becomes active once and stays so: birth[v] = the largest i <= n with u[v] > hf[i] (0: never), found by bisection of the
// ascending table hf.  Active at i <=> birth[v] >= i; the vertices with birth[v] == i are NEW at height i and are the only ones
// whose edges have to be hooked there (an edge between two older vertices was hooked at a higher height).
//
// Labelling is a lock-free union-find: parent[v] = v at the start; to unite a and b both roots are found (path halving on the way),
// the LARGER root is hooked under the smaller with a compare-and-swap that only succeeds while it still is a root, and a failed
// swap continues from the parent it saw.  parent[x] < x for every non-root, so there are no cycles, the root of a tree is its
// smallest vertex, and after all hooks of a height the trees are the components: the labels do not depend on the schedule and
// nothing waits for anything.  Every loop is bounded by M (each turn strictly lowers a vertex number); a loop that runs out --
// which a consistent forest cannot do -- raises the status word instead of returning a partial result.  Sizes are integer atomics
// (the lanes of a wave that share the first lane's root add once): exact in any order.  No float atomics anywhere.
//
// Arms:
//   on chip   M <= CL_LIM: one workgroup owns one permutation through ALL heights; birth, parent, count (int32) and acc (float64)
//             live in LDS, 20 bytes a vertex.  Global memory is read for t (twice), the CSR graph and the tables (L2, shared by
//             every workgroup) and written once at the end.  A height without new vertices skips labelling and counting.
//   streamed  larger M: the same state [Pb][M] in the caller's workspace; per height four launches -- hook, flatten (+ zero the
//             counts), count, accumulate -- between one prep and one final launch.  The kernel boundary is the only barrier.
#pragma clang fp contract(off)
#include <limits.h>

#include <utility>

#include "aug_draw.h"
#include "common.h"

namespace chebgcn {

constexpr int CL_LIM = 8160;                // vertices of the on-chip arm at most
constexpr int CL_LDS_VERTEX = 20;           // its LDS bytes per vertex
constexpr int CL_LDS_EXTRA = 512;           // ... and beside them (reduction scratch, flags)
constexpr int CL_SMAX = 4096;               // subjects
constexpr int CL_MMAX = 1 << 24;            // vertices
constexpr int CL_NHMAX = 1 << 16;           // heights
constexpr int CL_PBMAX = 65535;             // permutations of one call
constexpr int CL_T = 256;                   // threads of the streaming kernels
constexpr int CL_TBIG = 1024;               // threads of a workgroup that owns a permutation (CL_T while M <= CL_SMALL_M)
constexpr int CL_SMALL_M = 1024;
static_assert(CL_LIM * CL_LDS_VERTEX + CL_LDS_EXTRA <= 160 * 1024, "the on-chip state fits the LDS of a workgroup");

// how a forest is read and written: LDS of the workgroup, or global memory shared by the workgroups of a launch (loads and stores
// that pass the CU's own cache)
struct ClLds {
    static __device__ __forceinline__ int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    static __device__ __forceinline__ void st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    static __device__ __forceinline__ int cas(int* p, int expect, int v) {
        __hip_atomic_compare_exchange_strong(p, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return expect;
    }
    static __device__ __forceinline__ void add(int* p, int v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};
struct ClGlobal {
    static __device__ __forceinline__ int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ void st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ int cas(int* p, int expect, int v) {
        __hip_atomic_compare_exchange_strong(p, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expect;
    }
    static __device__ __forceinline__ void add(int* p, int v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

// a root-ward vertex of x with path halving: the root, unless other threads are hooking meanwhile (then a vertex that was one)
template <class Mem>
__device__ __forceinline__ int cl_find(int* parent, int x, int M, int& err) {
    for (int k = 0; k <= M; ++k) {          // x strictly falls
        const int p = Mem::ld(parent + x);
        if (p == x) return x;
        const int gp = Mem::ld(parent + p);
        if (gp == p) return p;
        Mem::st(parent + x, gp);
        x = gp;
    }
    err = CHEBGCN_CLUSTER_ELOOP;
    return x;
}

template <class Mem>
__device__ __forceinline__ void cl_unite(int* parent, int a, int b, int M, int& err) {
    for (int k = 0; k <= M; ++k) {          // the larger of the two roots strictly falls
        a = cl_find<Mem>(parent, a, M, err);
        b = cl_find<Mem>(parent, b, M, err);
        if (a == b || err) return;
        if (a < b) {
            const int s = a;
            a = b;
            b = s;
        }
        const int old = Mem::cas(parent + a, a, b);
        if (old == a) return;
        a = old;                            // somebody hooked a first: go on from where it hangs now
    }
    err = CHEBGCN_CLUSTER_ELOOP;
}

// the edges of a vertex that is new at height i, to every neighbour active there
template <class Mem>
__device__ __forceinline__ void cl_hook(const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx, int nnz, const int* birth,
                                        int* parent, int v, int i, int M, int& err) {
    const int e0 = min(max(ptr[v], 0), nnz), e1 = min(max(ptr[v + 1], e0), nnz);
    for (int e = e0; e < e1; ++e) {
        const int u = idx[e];
        if ((unsigned)u < (unsigned)M && u != v && birth[u] >= i) cl_unite<Mem>(parent, v, u, M, err);
    }
}

// count[r] += 1 for every lane with `act`; the lanes that share the first active lane's root add once.  Wave-uniform call.
template <class Mem>
__device__ __forceinline__ void cl_count_add(int* count, bool act, int r) {
    const unsigned long long m = __ballot(act);
    if (m == 0) return;
    const int lead = __ffsll((long long)m) - 1;
    const int r0 = __shfl(r, lead);
    const unsigned long long same = __ballot(act && r == r0);
    if (act) {
        if (r != r0) Mem::add(count + r, 1);
        else if ((int)(threadIdx.x & 63) == lead) Mem::add(count + r0, __popcll(same));
    }
}

// birth of a vertex of value u among the heights 1 .. n of the ascending table hf
__device__ __forceinline__ int cl_birth(float u, const float* __restrict__ hf, int n) {
    if (n < 1 || !(u > hf[1])) return 0;
    int lo = 1, hi = n;
    for (int k = 0; k < 32 && lo < hi; ++k) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (u > hf[mid]) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the maximum of `v` over the workgroup, the same value in every thread; red: 16 doubles of LDS, free again after the call
__device__ __forceinline__ double cl_block_max(double v, double* red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    const int nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = red[0];
    for (int w = 1; w < nw; ++w) r = fmax(r, red[w]);
    return r;
}

// heights of a permutation whose largest value is tmax: -1 = more than the NH the call carries
__device__ __forceinline__ int cl_heights(double tmax, double step, int NH, int mode) {
    if (mode == CHEBGCN_CLUSTER_EXTENT) return 1;
    if (!(tmax > 0.0)) return 0;
    const double nd = floor(__ddiv_rn(tmax, step));
    return nd <= (double)NH ? (int)nd : -1;
}

// ---- t ---------------------------------------------------------------------------------------------------------------------------
// block (256 vertices, permutation p0 + blockIdx.y)
__global__ void __launch_bounds__(CL_T)
signflip_t_kernel(const float* __restrict__ x, const double* __restrict__ q, const uint32_t* __restrict__ bits, float* __restrict__ t,
                  int S, int M, uint32_t p0, uint32_t seed) {
    __shared__ uint8_t neg[CL_SMAX];
    const int p = blockIdx.y;
    const uint32_t perm = p0 + (uint32_t)p;
    if (bits) {
        const uint32_t* row = bits + (size_t)p * ((S + 31) >> 5);
        for (int j = threadIdx.x; j < S; j += CL_T) neg[j] = (uint8_t)((row[j >> 5] >> (j & 31)) & 1u);
    } else {
        const AugKeys k = aug_keys(seed, 0u, perm);
        for (int j = threadIdx.x; j < S; j += CL_T) neg[j] = perm == 0u ? (uint8_t)0 : (uint8_t)(aug_draw(k, (uint32_t)j) >> 31);
    }
    __syncthreads();
    const int v = blockIdx.x * CL_T + threadIdx.x;
    if (v >= M) return;
    double s = 0.0;
    for (int j = 0; j < S; ++j) {
        const double xv = (double)x[(size_t)j * M + v];
        s = __dadd_rn(s, neg[j] ? -xv : xv);
    }
    const double m = __ddiv_rn(s, (double)S);
    const double d = __dsub_rn(q[v], __dmul_rn(s, m));
    float tv = 0.f;
    if (d > 0.0) tv = (float)__ddiv_rn(m, __dsqrt_rn(__ddiv_rn(d, (double)S * (double)(S - 1))));
    t[(size_t)p * M + v] = tv;
}

// ---- t of a permuted design (stats.design_test) ------------------------------------------------------------------------------------
// perm_glm_t<NJL>  the t of one contrast after the rows of the design's orthonormal basis Uf [S][r] were permuted (and subjects
//                  negated) by the caller's table: a[k] = sum_j Uf[row(p, j)][k] * (+-e[j][v]), then ssq = a.a, num = u.a,
//                  rss = q - ssq, t = num / sqrt(rss / dof * unorm2) -- float64, every multiply and add rounded on its own
//                  (include/chebgcn.h states them), so that NumPy restates it to the bit.
//                  Workgroup (PG_VB = 128 vertices, PT permutations), PG_NW waves: a lane owns TWO consecutive vertices and
//                  PTL = pg_ptl(r) permutations, wave w the permutations [w PTL, (w + 1) PTL) of the group -- a loaded value
//                  of e feeds PTL * NJ multiply-adds from registers, and the waves of a workgroup read the same rows of e at the
//                  same time (the CU's cache serves three of the four).  PTL falls with the rank: the accumulators (2 PTL NJ
//                  float64) and as many products in flight decide the occupancy, and beyond 4 waves a SIMD lost more than the
//                  saved loads gave (measured at S = 100, M = 10242, Pb = 256): 4 at r = 1, 2 up to r = 4, then 1.
//                  Rows of e are read vertex fastest, pg_u(NJ) rows in one go,
//                  no load behind a branch (a lane beyond M reads vertex M - 1 and drops it; M is any number, so a lane's two
//                  vertices are two 4-byte loads: a row of e need not start on 8 bytes).  The table entry and the row of Uf it
//                  names are the same for every lane: both addresses are functions of the permutation, j and k alone and come
//                  through the scalar cache; a row number >= S is clamped to S - 1 before it is an address.
//                  r > PG_PANEL runs in column panels of PG_PANEL, e re-read per panel (L2), ssq and num carried in registers
//                  across the panels so that k ascends overall; the LAST panel has NJL = r - PG_PANEL * (panels - 1) columns,
//                  a template argument (no multiply-add on padding).  A (permutation, vertex) result is a function of its own
//                  table row, e[:, v] and q[v] alone: the same bits whatever Pb, M or the batch holds.
#ifndef CG_PERM_NW
#define CG_PERM_NW 4
#endif
#ifndef CG_PERM_PTL1
#define CG_PERM_PTL1 4
#endif
#ifndef CG_PERM_PTL4
#define CG_PERM_PTL4 2
#endif
#ifndef CG_PERM_PTL
#define CG_PERM_PTL 1
#endif
#ifndef CG_PERM_U
#define CG_PERM_U 4
#endif
#ifndef CG_PERM_UWIDE
#define CG_PERM_UWIDE 1
#endif
constexpr int PG_NW = CG_PERM_NW;           // waves of a workgroup: permutations side by side on one vertex tile
constexpr int PG_V = 2;                     // consecutive vertices of a lane
constexpr int PG_VB = 64 * PG_V;            // vertices of a workgroup
constexpr int PG_PANEL = 16;                // columns of Uf of one pass over e
constexpr int PG_RMAX = 64;                 // rank of a design
// permutations of a lane, by the rank: a lane holds PTL * PG_V * min(r, PG_PANEL) float64 accumulators
constexpr int pg_ptl(int r) { return r <= 1 ? CG_PERM_PTL1 : r <= 4 ? CG_PERM_PTL4 : CG_PERM_PTL; }
// rows of e a lane loads in one go, by the columns of the panel
constexpr int pg_u(int nj) { return nj <= 8 ? CG_PERM_U : CG_PERM_UWIDE; }
constexpr int pg_pt(int r) { return PG_NW * pg_ptl(r); }    // permutations of a workgroup

__device__ __forceinline__ double pg_signed(double x, uint32_t flip) {      // flip: 0 or the sign bit
    return __hiloint2double(__double2hiint(x) ^ (int)flip, __double2loint(x));
}

// one row j of e into the accumulators of the lane's permutations: columns [k0, k0 + NJ) of the permuted rows of Uf
template <int PTL, int NJ>
__device__ __forceinline__ void pg_row(double (&a)[PTL][PG_V][NJ], const float (&y)[PG_V], const double* __restrict__ Ufk,
                                       const uint32_t* const (&rw)[PTL], int j, int S, int r) {
    double yd[PG_V];
#pragma unroll
    for (int v = 0; v < PG_V; ++v) yd[v] = (double)y[v];
#pragma unroll
    for (int i = 0; i < PTL; ++i) {
        const uint32_t ent = rw[i][j];
        const uint32_t row = min(ent & 0x7FFFFFFFu, (uint32_t)(S - 1));
        const uint32_t flip = ent & 0x80000000u;
        const double* __restrict__ ur = Ufk + (size_t)row * r;
        double x[PG_V];
#pragma unroll
        for (int v = 0; v < PG_V; ++v) x[v] = pg_signed(yd[v], flip);
#pragma unroll
        for (int k = 0; k < NJ; ++k) {
            const double uk = ur[k];
#pragma unroll
            for (int v = 0; v < PG_V; ++v) a[i][v][k] = __dadd_rn(a[i][v][k], __dmul_rn(uk, x[v]));
        }
    }
}

// one panel: the pass over e, then its columns' share of ssq and num (k ascending)
template <int PTL, int NJ>
__device__ __forceinline__ void pg_panel(double (&ssq)[PTL][PG_V], double (&num)[PTL][PG_V], const float* __restrict__ e,
                                         const double* __restrict__ Ufk, const double* __restrict__ uk0,
                                         const uint32_t* const (&rw)[PTL], int S, int M, int r, int i0, int i1) {
    constexpr int PG_U = pg_u(NJ);
    double a[PTL][PG_V][NJ];
#pragma unroll
    for (int i = 0; i < PTL; ++i)
#pragma unroll
        for (int v = 0; v < PG_V; ++v)
#pragma unroll
            for (int k = 0; k < NJ; ++k) a[i][v][k] = 0.0;
    for (int j = 0; j < S; j += PG_U) {
        float y[PG_U][PG_V];
#pragma unroll
        for (int s = 0; s < PG_U; ++s) {
            const float* row = e + (size_t)min(j + s, S - 1) * M;
            y[s][0] = row[i0];
            y[s][1] = row[i1];
        }
        if (j + PG_U <= S) {
#pragma unroll
            for (int s = 0; s < PG_U; ++s) pg_row<PTL, NJ>(a, y[s], Ufk, rw, j + s, S, r);
        } else {
#pragma unroll
            for (int s = 0; s < PG_U; ++s)
                if (j + s < S) pg_row<PTL, NJ>(a, y[s], Ufk, rw, j + s, S, r);
        }
    }
#pragma unroll
    for (int k = 0; k < NJ; ++k) {
        const double uk = uk0[k];
#pragma unroll
        for (int i = 0; i < PTL; ++i)
#pragma unroll
            for (int v = 0; v < PG_V; ++v) {
                ssq[i][v] = __dadd_rn(ssq[i][v], __dmul_rn(a[i][v][k], a[i][v][k]));
                num[i][v] = __dadd_rn(num[i][v], __dmul_rn(uk, a[i][v][k]));
            }
    }
}

// block (PG_VB vertices, permutations [blockIdx.y PT, + PT)), PG_NW waves.  MORE: r = PG_PANEL * (panels - 1) + NJL with at least
// one full panel before the last; else r = NJL
template <int NJL, bool MORE>
__global__ void __launch_bounds__(PG_NW * 64)
perm_glm_t_kernel(const float* __restrict__ e, const double* __restrict__ q, const double* __restrict__ Uf,
                  const double* __restrict__ u, double unorm2, double dof, const uint32_t* __restrict__ rows, float* __restrict__ t,
                  int S, int M, int r, int Pb) {
    constexpr int PTL = pg_ptl(MORE ? PG_PANEL + NJL : NJL);
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m0 = blockIdx.x * PG_VB + lane * PG_V;
    const int pb = (blockIdx.y * PG_NW + w) * PTL;
    if (pb >= Pb) return;                                   // (the same in every lane of the wave; no barrier follows)
    const int i0 = min(m0, M - 1), i1 = min(m0 + 1, M - 1);
    const uint32_t* rw[PTL];                                // a permutation beyond Pb computes the last one again and stores nothing
#pragma unroll
    for (int i = 0; i < PTL; ++i) rw[i] = rows + (size_t)min(pb + i, Pb - 1) * S;
    double ssq[PTL][PG_V], num[PTL][PG_V];
#pragma unroll
    for (int i = 0; i < PTL; ++i)
#pragma unroll
        for (int v = 0; v < PG_V; ++v) ssq[i][v] = num[i][v] = 0.0;
    int k0 = 0;
    if (MORE)
        for (; k0 < r - NJL; k0 += PG_PANEL) pg_panel<PTL, PG_PANEL>(ssq, num, e, Uf + k0, u + k0, rw, S, M, r, i0, i1);
    pg_panel<PTL, NJL>(ssq, num, e, Uf + k0, u + k0, rw, S, M, r, i0, i1);

    const double floor_ = __dmul_rn(4.0 * (double)(S + r), 0x1p-53);
    const double qv[PG_V] = {q[i0], q[i1]};
#pragma unroll
    for (int i = 0; i < PTL; ++i) {
        if (pb + i >= Pb) break;
#pragma unroll
        for (int v = 0; v < PG_V; ++v) {
            double rss = __dsub_rn(qv[v], ssq[i][v]);
            if (rss < __dmul_rn(floor_, qv[v])) rss = 0.0;  // round-off of the subtraction (also a negative one)
            const double var = __dmul_rn(__ddiv_rn(rss, dof), unorm2);
            float tv = 0.f;
            if (var > 0.0) tv = (float)__ddiv_rn(num[i][v], __dsqrt_rn(var));
            if (m0 + v < M) t[(size_t)(pb + i) * M + m0 + v] = tv;
        }
    }
}

template <int NJL, bool MORE>
static void perm_glm_launch(hipStream_t stream, const float* e, const double* q, const double* Uf, const double* u, double unorm2,
                            double dof, const uint32_t* rows, float* t, int S, int M, int r, int Pb) {
    static char name[48];
    static const int named = snprintf(name, sizeof name, "perm_glm_t_kernel<%d, %s>", NJL, MORE ? "panels" : "one");
    (void)named;
    note_dispatch(name);
    const int PT = pg_pt(r);
    const dim3 grid((unsigned)((M + PG_VB - 1) / PG_VB), (unsigned)((Pb + PT - 1) / PT));
    hipLaunchKernelGGL((perm_glm_t_kernel<NJL, MORE>), grid, dim3(PG_NW * 64), 0, stream, e, q, Uf, u, unorm2, dof, rows, t, S, M, r,
                       Pb);
}

typedef void (*PermGlmLaunch)(hipStream_t, const float*, const double*, const double*, const double*, double, double, const uint32_t*,
                              float*, int, int, int, int);
template <int... NJ>
static PermGlmLaunch perm_glm_launch_of(int r, std::integer_sequence<int, NJ...>) {
    static const PermGlmLaunch one[] = {perm_glm_launch<NJ + 1, false>...};
    static const PermGlmLaunch more[] = {perm_glm_launch<NJ + 1, true>...};
    const int njl = r - PG_PANEL * ((r - 1) / PG_PANEL);
    return (r > PG_PANEL ? more : one)[njl - 1];
}

// ---- the on-chip arm ----------------------------------------------------------------------------------------------------------------
// block: permutation blockIdx.x
__global__ void __launch_bounds__(CL_TBIG)
cluster_onchip_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx, int nnz, const float* __restrict__ t, float sgn,
                      const float* __restrict__ hf, const double* __restrict__ hw, int NH, const double* __restrict__ ep, double step,
                      double* __restrict__ out, int32_t* __restrict__ labels, double* __restrict__ pmax, int32_t* status, int M,
                      int mode) {
    extern __shared__ __attribute__((aligned(16))) char cl_smem[];
    double* acc = reinterpret_cast<double*>(cl_smem);       // [M]
    double* red = acc + M;                                  // [16]
    int* birth = reinterpret_cast<int*>(red + 16);          // [M]
    int* parent = birth + M;                                // [M]
    int* count = parent + M;                                // [M]
    int* flag = count + M;                                  // [0], [1]: a vertex is new at a height of that parity; [2]: error
    const int tid = threadIdx.x, nt = blockDim.x;
    const float* tp = t + (size_t)blockIdx.x * M;

    double mx = -INFINITY;
    for (int v = tid; v < M; v += nt) mx = fmax(mx, (double)(sgn * tp[v]));
    if (tid < 3) flag[tid] = 0;
    const double tmax = cl_block_max(mx, red);
    const int n = cl_heights(tmax, step, NH, mode);
    if (n < 0) {                                            // (the same in every thread)
        if (tid == 0) atomicMax(status, (int)CHEBGCN_CLUSTER_EHEIGHTS);
        return;
    }
    for (int v = tid; v < M; v += nt) {
        birth[v] = cl_birth(sgn * tp[v], hf, n);
        parent[v] = v;
        count[v] = 0;
        acc[v] = 0.0;
    }
    __syncthreads();

    for (int i = n; i >= 1; --i) {
        int err = 0;
        bool mine = false;
        for (int v = tid; v < M; v += nt)
            if (birth[v] == i) {
                mine = true;
                cl_hook<ClLds>(ptr, idx, nnz, birth, parent, v, i, M, err);
            }
        if (mine) flag[i & 1] = 1;
        if (err) flag[2] = err;
        __syncthreads();
        if (flag[2]) break;
        if (tid == 0) flag[(i + 1) & 1] = 0;                // (last read behind the barrier of the height before)
        if (flag[i & 1]) {                                  // new vertices: the components and their sizes change
            for (int v = tid; v < M; v += nt) {
                count[v] = 0;
                if (birth[v] >= i) {
                    int r = v;
                    for (int k = 0; k <= M; ++k) {
                        const int p = ClLds::ld(parent + r);
                        if (p == r) break;
                        r = p;
                        if (k == M) err = CHEBGCN_CLUSTER_ELOOP;
                    }
                    ClLds::st(parent + v, r);
                }
            }
            if (err) flag[2] = err;
            __syncthreads();
            if (flag[2]) break;
            for (int v0 = 0; v0 < M; v0 += nt) {
                const int v = v0 + tid;
                const bool act = v < M && birth[v] >= i;
                cl_count_add<ClLds>(count, act, act ? parent[v] : 0);
            }
            __syncthreads();
        }
        const double w = hw[i];
        for (int v = tid; v < M; v += nt)
            if (birth[v] >= i) acc[v] = __dadd_rn(acc[v], __dmul_rn(ep[count[parent[v]]], w));
        __syncthreads();                                    // the next height's hooks rewrite parent
    }
    if (flag[2]) {
        if (tid == 0) atomicMax(status, flag[2]);
        return;
    }
    mx = 0.0;
    for (int v = tid; v < M; v += nt) {
        const double a = acc[v];
        mx = fmax(mx, a);
        if (out) out[(size_t)blockIdx.x * M + v] = a;
        if (labels) labels[(size_t)blockIdx.x * M + v] = birth[v] >= 1 ? parent[v] : -1;
    }
    if (pmax) {
        mx = cl_block_max(mx, red);
        if (tid == 0) pmax[blockIdx.x] = mx;
    }
}

// ---- the streamed arm ---------------------------------------------------------------------------------------------------------------
struct ClState {            // [Pb][M] each, in the workspace
    double* acc;
    int* birth;
    int* parent;
    int* count;
};

// block: permutation blockIdx.x
__global__ void __launch_bounds__(CL_TBIG)
cluster_prep_kernel(const float* __restrict__ t, float sgn, const float* __restrict__ hf, int NH, double step, ClState st, int32_t* status,
                    int M, int mode) {
    __shared__ double red[16];
    const size_t o = (size_t)blockIdx.x * M;
    double mx = -INFINITY;
    for (int v = threadIdx.x; v < M; v += blockDim.x) mx = fmax(mx, (double)(sgn * t[o + v]));
    int n = cl_heights(cl_block_max(mx, red), step, NH, mode);
    if (n < 0) {
        if (threadIdx.x == 0) atomicMax(status, (int)CHEBGCN_CLUSTER_EHEIGHTS);
        n = 0;                                              // (the call's result is void: the status says so)
    }
    for (int v = threadIdx.x; v < M; v += blockDim.x) {
        st.birth[o + v] = cl_birth(sgn * t[o + v], hf, n);
        st.parent[o + v] = v;
        st.count[o + v] = 0;
        st.acc[o + v] = 0.0;
    }
}

// block (256 vertices, permutation blockIdx.y), in the four kernels of a height
__global__ void __launch_bounds__(CL_T)
cluster_hook_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx, int nnz, ClState st, int32_t* status, int M, int i) {
    const int v = blockIdx.x * CL_T + threadIdx.x;
    if (v >= M) return;
    const size_t o = (size_t)blockIdx.y * M;
    if (st.birth[o + v] != i) return;
    int err = 0;
    cl_hook<ClGlobal>(ptr, idx, nnz, st.birth + o, st.parent + o, v, i, M, err);
    if (err) atomicMax(status, err);
}

__global__ void __launch_bounds__(CL_T)
cluster_flatten_kernel(ClState st, int32_t* status, int M, int i) {
    const int v = blockIdx.x * CL_T + threadIdx.x;
    if (v >= M) return;
    const size_t o = (size_t)blockIdx.y * M;
    st.count[o + v] = 0;
    if (st.birth[o + v] < i) return;
    int* parent = st.parent + o;
    int r = v;
    for (int k = 0; k <= M; ++k) {
        const int p = ClGlobal::ld(parent + r);
        if (p == r) break;
        r = p;
        if (k == M) atomicMax(status, (int)CHEBGCN_CLUSTER_ELOOP);
    }
    ClGlobal::st(parent + v, r);
}

__global__ void __launch_bounds__(CL_T)
cluster_count_kernel(ClState st, int M, int i) {
    const int v = blockIdx.x * CL_T + threadIdx.x;
    const size_t o = (size_t)blockIdx.y * M;
    const bool act = v < M && st.birth[o + v] >= i;
    cl_count_add<ClGlobal>(st.count + o, act, act ? st.parent[o + v] : 0);
}

__global__ void __launch_bounds__(CL_T)
cluster_accum_kernel(ClState st, const double* __restrict__ hw, const double* __restrict__ ep, int M, int i) {
    const int v = blockIdx.x * CL_T + threadIdx.x;
    if (v >= M) return;
    const size_t o = (size_t)blockIdx.y * M;
    if (st.birth[o + v] < i) return;
    const int c = min(max(st.count[o + st.parent[o + v]], 0), M);
    st.acc[o + v] = __dadd_rn(st.acc[o + v], __dmul_rn(ep[c], hw[i]));
}

// block: permutation blockIdx.x.  st.acc == NULL: the plain map u (mode MAX), no state at all
__global__ void __launch_bounds__(CL_TBIG)
cluster_final_kernel(ClState st, const float* __restrict__ t, float sgn, double* __restrict__ out, int32_t* __restrict__ labels,
                     double* __restrict__ pmax, int M) {
    __shared__ double red[16];
    const size_t o = (size_t)blockIdx.x * M;
    double mx = -INFINITY;
    for (int v = threadIdx.x; v < M; v += blockDim.x) {
        const double a = st.acc ? st.acc[o + v] : (double)(sgn * t[o + v]);
        mx = fmax(mx, a);
        if (out) out[o + v] = a;
        if (labels) labels[o + v] = (st.acc && st.birth[o + v] >= 1) ? st.parent[o + v] : -1;
    }
    if (pmax) {
        mx = cl_block_max(mx, red);
        if (threadIdx.x == 0) pmax[blockIdx.x] = mx;
    }
}

static inline size_t cl_ws_bytes(int Pb, int M) { return (size_t)Pb * M * CL_LDS_VERTEX; }
static inline bool cl_sizes_ok(int Pb, int M) { return Pb >= 1 && Pb <= CL_PBMAX && M >= 1 && M <= CL_MMAX; }
static inline int cl_wg(int M) { return M <= CL_SMALL_M ? CL_T : CL_TBIG; }

}  // namespace chebgcn

using namespace chebgcn;

extern "C" int chebgcn_cluster_query(int what) {
    switch (what) {
        case 0: return CL_LIM;              // vertices of the on-chip arm at most
        case 1: return CL_SMAX;             // subjects
        case 2: return CL_MMAX;             // vertices
        case 3: return CL_NHMAX;            // heights
        case 4: return CL_PBMAX;            // permutations of one call
        case 5: return CL_LDS_VERTEX;       // bytes of state per (permutation, vertex): LDS on chip, workspace streamed
        default: return -1;
    }
}

extern "C" size_t chebgcn_cluster_enhance_workspace(int Pb, int M, int mode, int arm) {
    if (!cl_sizes_ok(Pb, M) || mode == CHEBGCN_CLUSTER_MAX || arm < 0 || arm > 2) return 0;
    if (arm == 1 || (arm == 0 && M <= CL_LIM)) return 0;
    return cl_ws_bytes(Pb, M);
}

extern "C" int chebgcn_signflip_t(const float* x, const double* q, const uint32_t* bits, float* t, int S, int M, uint32_t p0, int Pb,
                                  uint32_t seed, chebgcn_stream stream_) {
    CG_REQUIRE(x && q && t, "signflip_t: NULL argument");
    CG_REQUIRE(S >= 2 && M >= 1 && Pb >= 1, "signflip_t: bad shape (S = %d, M = %d, Pb = %d)", S, M, Pb);
    if (S > CL_SMAX || M > CL_MMAX || Pb > CL_PBMAX)
        return fail(CHEBGCN_EUNSUPPORTED, "signflip_t: S = %d, M = %d, Pb = %d; served: S <= %d, M <= %d, Pb <= %d", S, M, Pb, CL_SMAX,
                    CL_MMAX, CL_PBMAX);
    CG_REQUIRE((((uintptr_t)x | (uintptr_t)t | (uintptr_t)bits) & 3) == 0 && ((uintptr_t)q & 7) == 0, "signflip_t: unaligned argument");
    note_dispatch("signflip_t_kernel");
    const dim3 grid((unsigned)((M + CL_T - 1) / CL_T), (unsigned)Pb);
    hipLaunchKernelGGL(signflip_t_kernel, grid, dim3(CL_T), 0, (hipStream_t)stream_, x, q, bits, t, S, M, p0, seed);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_perm_glm_query(int what) {
    if (what > 100 && what <= 100 + PG_RMAX) return pg_pt(what - 100);      // permutations of a workgroup at rank what - 100
    switch (what) {
        case 0: return PG_VB;               // vertices of a workgroup
        case 1: return pg_pt(1);            // permutations of a workgroup at most
        case 2: return PG_PANEL;            // columns of Uf of one pass over e
        case 3: return PG_RMAX;             // rank of a design
        case 4: return CL_SMAX;             // subjects
        case 5: return CL_MMAX;             // vertices
        case 6: return CL_PBMAX;            // permutations of one call
        default: return -1;
    }
}

extern "C" int chebgcn_perm_glm_t(const float* e, const double* q, const double* Uf, const double* u, double unorm2, int dof,
                                  const uint32_t* rows, float* t, int S, int M, int r, int Pb, chebgcn_stream stream_) {
    CG_REQUIRE(e && q && Uf && u && rows && t, "perm_glm_t: NULL argument");
    CG_REQUIRE(S >= 2 && M >= 1 && Pb >= 1 && r >= 1, "perm_glm_t: bad shape (S = %d, M = %d, r = %d, Pb = %d)", S, M, r, Pb);
    if (S > CL_SMAX || M > CL_MMAX || Pb > CL_PBMAX || r > PG_RMAX)
        return fail(CHEBGCN_EUNSUPPORTED, "perm_glm_t: S = %d, M = %d, Pb = %d, r = %d; served: S <= %d, M <= %d, Pb <= %d, r <= %d", S,
                    M, Pb, r, CL_SMAX, CL_MMAX, CL_PBMAX, PG_RMAX);
    CG_REQUIRE(r < S && dof >= 1, "perm_glm_t: r = %d of S = %d subjects, dof = %d", r, S, dof);
    CG_REQUIRE((((uintptr_t)e | (uintptr_t)t | (uintptr_t)rows) & 3) == 0 && (((uintptr_t)q | (uintptr_t)Uf | (uintptr_t)u) & 7) == 0,
               "perm_glm_t: unaligned argument");
    CG_REQUIRE(unorm2 > 0.0 && unorm2 <= 1.7976931348623157e308, "perm_glm_t: unorm2 = %g", unorm2);
    perm_glm_launch_of(r, std::make_integer_sequence<int, PG_PANEL>())((hipStream_t)stream_, e, q, Uf, u, unorm2, (double)dof, rows, t,
                                                                      S, M, r, Pb);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_cluster_enhance(const int32_t* ptr, const int32_t* idx, int64_t nnz, const float* t, int negate,
                                       const float* hf, const double* hw, int NH, const double* ep, double step, double* out,
                                       int32_t* labels, double* pmax, int32_t* status, void* workspace, size_t workspace_bytes,
                                       int Pb, int M, int mode, int arm, chebgcn_stream stream_) {
    CG_REQUIRE(t && (out || pmax || labels), "cluster_enhance: NULL argument");
    CG_REQUIRE(mode == CHEBGCN_CLUSTER_MAX || mode == CHEBGCN_CLUSTER_EXTENT || mode == CHEBGCN_CLUSTER_TFCE,
               "cluster_enhance: unknown mode %d", mode);
    CG_REQUIRE(arm >= 0 && arm <= 2, "cluster_enhance: arm = %d (0 automatic, 1 on chip, 2 streamed)", arm);
    CG_REQUIRE(Pb >= 1 && M >= 1, "cluster_enhance: bad shape (Pb = %d, M = %d)", Pb, M);
    if (!cl_sizes_ok(Pb, M))
        return fail(CHEBGCN_EUNSUPPORTED, "cluster_enhance: Pb = %d, M = %d; served: Pb <= %d, M <= %d", Pb, M, CL_PBMAX, CL_MMAX);
    CG_REQUIRE((((uintptr_t)t | (uintptr_t)labels) & 3) == 0 && (((uintptr_t)out | (uintptr_t)pmax) & 7) == 0,
               "cluster_enhance: unaligned argument");
    hipStream_t stream = (hipStream_t)stream_;
    const float sgn = negate ? -1.f : 1.f;
    ClState st{nullptr, nullptr, nullptr, nullptr};
    if (mode == CHEBGCN_CLUSTER_MAX) {
        note_dispatch("cluster_final_kernel<plain>");
        hipLaunchKernelGGL(cluster_final_kernel, dim3(Pb), dim3(cl_wg(M)), 0, stream, st, t, sgn, out, nullptr, pmax, M);
        CG_HIP(hipGetLastError());
        return CHEBGCN_OK;
    }
    CG_REQUIRE(nnz >= 0 && nnz <= INT_MAX, "cluster_enhance: nnz = %lld", (long long)nnz);
    CG_REQUIRE(ptr && (idx || nnz == 0) && hf && hw && ep && status, "cluster_enhance: NULL argument");
    CG_REQUIRE(NH >= 1, "cluster_enhance: NH = %d heights", NH);
    if (NH > CL_NHMAX) return fail(CHEBGCN_EUNSUPPORTED, "cluster_enhance: NH = %d heights, at most %d", NH, CL_NHMAX);
    CG_REQUIRE(mode == CHEBGCN_CLUSTER_EXTENT || (step > 0.0 && step <= 1.7976931348623157e308), "cluster_enhance: step = %g", step);
    CG_REQUIRE((((uintptr_t)ptr | (uintptr_t)idx | (uintptr_t)hf | (uintptr_t)status) & 3) == 0 &&
                   (((uintptr_t)hw | (uintptr_t)ep) & 7) == 0,
               "cluster_enhance: unaligned argument");
    if (arm == 1 && M > CL_LIM)
        return fail(CHEBGCN_EUNSUPPORTED, "cluster_enhance: the on-chip arm serves M <= %d, not %d", CL_LIM, M);
    if (arm == 1 || (arm == 0 && M <= CL_LIM)) {
        const size_t lds = (size_t)M * CL_LDS_VERTEX + CL_LDS_EXTRA;
        CG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(cluster_onchip_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
        note_dispatch("cluster_onchip_kernel");
        hipLaunchKernelGGL(cluster_onchip_kernel, dim3(Pb), dim3(cl_wg(M)), lds, stream, ptr, idx, (int)nnz, t, sgn, hf, hw, NH, ep,
                           step, out, labels, pmax, status, M, mode);
        CG_HIP(hipGetLastError());
        return CHEBGCN_OK;
    }
    const size_t need = cl_ws_bytes(Pb, M);
    CG_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 15) == 0,
               "cluster_enhance: the streamed arm needs %zu bytes of 16-byte aligned workspace, got %zu", need, workspace_bytes);
    const size_t cells = (size_t)Pb * M;
    st.acc = static_cast<double*>(workspace);
    st.birth = reinterpret_cast<int*>(st.acc + cells);
    st.parent = st.birth + cells;
    st.count = st.parent + cells;
    const int heights = mode == CHEBGCN_CLUSTER_EXTENT ? 1 : NH;
    const dim3 grid((unsigned)((M + CL_T - 1) / CL_T), (unsigned)Pb);
    note_dispatch("cluster_prep_kernel");
    hipLaunchKernelGGL(cluster_prep_kernel, dim3(Pb), dim3(CL_TBIG), 0, stream, t, sgn, hf, NH, step, st, status, M, mode);
    note_dispatch_more("cluster_hook_kernel");
    note_dispatch_more("cluster_flatten_kernel");
    note_dispatch_more("cluster_count_kernel");
    note_dispatch_more("cluster_accum_kernel");
    for (int i = heights; i >= 1; --i) {
        hipLaunchKernelGGL(cluster_hook_kernel, grid, dim3(CL_T), 0, stream, ptr, idx, (int)nnz, st, status, M, i);
        hipLaunchKernelGGL(cluster_flatten_kernel, grid, dim3(CL_T), 0, stream, st, status, M, i);
        hipLaunchKernelGGL(cluster_count_kernel, grid, dim3(CL_T), 0, stream, st, M, i);
        hipLaunchKernelGGL(cluster_accum_kernel, grid, dim3(CL_T), 0, stream, st, hw, ep, M, i);
    }
    note_dispatch_more("cluster_final_kernel<state>");
    hipLaunchKernelGGL(cluster_final_kernel, dim3(Pb), dim3(CL_TBIG), 0, stream, st, t, sgn, out, labels, pmax, M);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}
