// Graph filters (filters.GraphFilter): y[j] = h_j(L) x = sum_{k<K} coeff[j][k] T_k(L~) x for up to FILTER_JMAX filters at once,
// on the recurrence T_0 = x, T_1 = L~ x, T_k = 2 L~ T_{k-1} - T_{k-2} of the conv layers -- with FIXED coefficients, so that no
// contraction is needed and, in the rolling arm, no stack either.
//
//   rolling arm  cheb_filter_step_kernel<P>: one launch per order k = 1 .. K-1.  A thread owns one row of L~ for P consecutive
//                planes: the row's indices and values (the handle's CSR in the caller's entry order) are loaded once and used
//                for P planes, the row sum is one fmaf chain in CSR order from 0, T_k = 2 * sum - T_{k-2} is formed in
//                registers, stored where T_{k-2} lay (same element, same thread) and added into the J accumulators
//                y[j] = fmaf(coeff[j][k], T_k, y[j]).  Two work slabs whatever K and J are; x is T_0 and is never written.
//   stack arm    the recurrence dispatch of chebgcn_recurrence_fwd into a K-slab stack (the on-chip / ordered kernels, which beat
//                any launch-per-step scheme where they exist), then cheb_filter_mix_kernel<NJ>: one streaming pass over the flat
//                slab, 16 bytes per access, every stack element read once for all J filters.
//
// Both arms sum over k in ascending order, y = coeff[j][0] * x (a rounded product) and then one fmaf per order: what differs
// between them is the order inside a row sum of L~ (CSR order here, the image's order in the recurrence kernels).
// A plane's result depends on nothing but that plane: not on P, on its neighbours in the group, or on the grid.
#include "common.h"

namespace chebgcn {

constexpr int FILTER_JMAX = 8;
constexpr int FILTER_KMAX = 256;
constexpr int FILTER_T = 256;               // threads: one row each
constexpr int FILTER_GROUPS_Y = 65535;      // plane groups of a grid at most: a workgroup loops over the rest
constexpr int FILTER_MIX_GRID = 8192;       // workgroups of the mix pass at most: a thread loops over its pieces

// k == 0: the scale pass of K == 1 (y[j] = coeff[j][0] * x, no gather, nothing stored but y).
// k == 1: src == x, no sub; y[j] starts as coeff[j][0] * x.  k >= 2: out may alias sub (element-wise, same thread), never src.
template <int P>
__global__ void __launch_bounds__(FILTER_T)
cheb_filter_step_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ val,
                        const float* __restrict__ x, const float* src, const float* sub, float* out,
                        const float* __restrict__ coeff, float* __restrict__ y, int M, int Mp, int nplanes, int ngroups, int k,
                        int K, int J) {
    const int r = blockIdx.x * FILTER_T + threadIdx.x;
    if (r >= M) return;
    const size_t yslab = (size_t)nplanes * Mp;
    const int e0 = k ? rowptr[r] : 0, e1 = k ? rowptr[r + 1] : 0;
    for (int grp = blockIdx.y; grp < ngroups; grp += gridDim.y) {
        const int p0 = grp * P;
        const int np = min(P, nplanes - p0);            // the last group may be partial
        const size_t base = (size_t)p0 * Mp;
        float t[P];
#pragma unroll
        for (int p = 0; p < P; ++p) t[p] = 0.f;
        for (int e = e0; e < e1; ++e) {
            const int c = col[e];
            const float v = val[e];
#pragma unroll
            for (int p = 0; p < P; ++p)
                if (p < np) t[p] = fmaf(v, src[base + (size_t)p * Mp + c], t[p]);
        }
        float x0[P];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            x0[p] = 0.f;
            if (p < np) {
                const size_t at = base + (size_t)p * Mp + r;
                if (k <= 1) x0[p] = x[at];
                if (k == 0) t[p] = x0[p];
                if (k >= 2) t[p] = 2.f * t[p] - sub[at];
                if (k >= 1) out[at] = t[p];
            }
        }
        for (int j = 0; j < J; ++j) {
            const float c0 = coeff[(size_t)j * K], ck = coeff[(size_t)j * K + k];
#pragma unroll
            for (int p = 0; p < P; ++p) {
                if (p < np) {
                    float* yp = y + (size_t)j * yslab + base + (size_t)p * Mp + r;
                    if (k == 0) *yp = __fmul_rn(c0, x0[p]);
                    else if (k == 1) *yp = fmaf(ck, t[p], __fmul_rn(c0, x0[p]));
                    else *yp = fmaf(ck, t[p], *yp);
                }
            }
        }
    }
}

// y[j][i] = sum_k coeff[j][k] * stack[k][i] over the n4 16-byte pieces of a slab (pad included: scratch in, scratch out)
template <int NJ>
__global__ void __launch_bounds__(256)
cheb_filter_mix_kernel(const float4* __restrict__ stack, const float* __restrict__ coeff, float4* __restrict__ y, size_t n4, int K) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        float4 acc[NJ];
        const float4 t0 = stack[i];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const float c = coeff[(size_t)j * K];
            acc[j] = make_float4(__fmul_rn(c, t0.x), __fmul_rn(c, t0.y), __fmul_rn(c, t0.z), __fmul_rn(c, t0.w));
        }
        for (int k = 1; k < K; ++k) {
            const float4 t = stack[(size_t)k * n4 + i];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const float c = coeff[(size_t)j * K + k];
                acc[j].x = fmaf(c, t.x, acc[j].x);
                acc[j].y = fmaf(c, t.y, acc[j].y);
                acc[j].z = fmaf(c, t.z, acc[j].z);
                acc[j].w = fmaf(c, t.w, acc[j].w);
            }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) y[(size_t)j * n4 + i] = acc[j];
    }
}

template <int P>
static void launch_step(const chebgcn_graph* g, const float* x, const float* src, const float* sub, float* out, const float* coeff,
                        float* y, int nplanes, int k, int K, int J, hipStream_t stream) {
    const int ngroups = (nplanes + P - 1) / P;
    const dim3 grid((unsigned)((g->M + FILTER_T - 1) / FILTER_T), (unsigned)(ngroups < FILTER_GROUPS_Y ? ngroups : FILTER_GROUPS_Y));
    hipLaunchKernelGGL(cheb_filter_step_kernel<P>, grid, dim3(FILTER_T), 0, stream, g->fwd.rowptr, g->fwd.col32, g->fwd.cval, x, src,
                       sub, out, coeff, y, g->M, g->Mp, nplanes, ngroups, k, K, J);
}

static int filter_rolling(const chebgcn_graph* g, const float* x, const float* coeff, float* y, float* work, int nplanes, int K,
                          int J, hipStream_t stream) {
    const bool four = nplanes >= 4;
    note_dispatch(four ? "cheb_filter_step_kernel<4>" : "cheb_filter_step_kernel<1>");
    const size_t slab = (size_t)nplanes * g->Mp;
    // T_k goes to work[(k - 1) & 1]: T_1 -> work 0, T_2 -> work 1 (T_0 is x, which stays), T_3 over T_1, T_4 over T_2, ...
    for (int k = K == 1 ? 0 : 1; k < (K == 1 ? 1 : K); ++k) {
        const float* src = k <= 1 ? x : work + (size_t)(k & 1) * slab;                         // T_{k-1}
        const float* sub = k < 2 ? nullptr : (k == 2 ? x : work + (size_t)((k - 1) & 1) * slab);  // T_{k-2}
        float* out = k == 0 ? nullptr : work + (size_t)((k - 1) & 1) * slab;
        if (four) launch_step<4>(g, x, src, sub, out, coeff, y, nplanes, k, K, J, stream);
        else launch_step<1>(g, x, src, sub, out, coeff, y, nplanes, k, K, J, stream);
    }
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

static int filter_stack(const chebgcn_graph* g, const float* x, const float* coeff, float* y, float* stack, int nplanes, int K, int J,
                        hipStream_t stream) {
    const float* src = x;                   // K == 1: the stack is x itself
    if (K > 1) {
        const int rc = chebgcn_recurrence_fwd(g, x, stack, 1, nplanes, K, (chebgcn_stream)stream);
        if (rc != CHEBGCN_OK) return rc;
        note_dispatch_more("cheb_filter_mix_kernel");
        src = stack;
    } else {
        note_dispatch("cheb_filter_mix_kernel");
    }
    const size_t n4 = (size_t)nplanes * g->Mp / 4;
    const size_t nblk = (n4 + 255) / 256;
    const dim3 grid((unsigned)(nblk < (size_t)FILTER_MIX_GRID ? nblk : (size_t)FILTER_MIX_GRID));
#define CG_MIX(NJ)                                                                                                  \
    case NJ:                                                                                                        \
        hipLaunchKernelGGL(cheb_filter_mix_kernel<NJ>, grid, dim3(256), 0, stream, (const float4*)src, coeff, (float4*)y, n4, K); \
        break
    switch (J) {
        CG_MIX(1); CG_MIX(2); CG_MIX(3); CG_MIX(4); CG_MIX(5); CG_MIX(6); CG_MIX(7); CG_MIX(8);
    }
#undef CG_MIX
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

// 1 rolling, 2 stack, 0 bad arguments
static int filter_arm(const chebgcn_graph* g, int K, int arm) {
    if (arm == 0) return (K > 1 && (g->lds_ok || g->ord_ok)) ? 2 : 1;
    return arm;
}

static bool filter_shape_ok(int nplanes, int K, int J, int arm) {
    return nplanes >= 1 && nplanes < (1 << 30) && K >= 1 && K <= FILTER_KMAX && J >= 1 && J <= FILTER_JMAX && arm >= 0 && arm <= 2;
}

}  // namespace chebgcn

using namespace chebgcn;

extern "C" size_t chebgcn_cheb_filter_workspace(const chebgcn_graph* g, int nplanes, int K, int J, int arm) {
    if (!g || !filter_shape_ok(nplanes, K, J, arm)) return 0;
    const size_t slab = (size_t)nplanes * g->Mp * sizeof(float);
    return filter_arm(g, K, arm) == 2 ? (size_t)K * slab : 2 * slab;
}

extern "C" int chebgcn_cheb_filter(const chebgcn_graph* g, const float* x, const float* coeff, float* y, void* workspace,
                                   int nplanes, int K, int J, int arm, chebgcn_stream stream_) {
    CG_REQUIRE(K >= 1 && K <= FILTER_KMAX, "cheb_filter: K = %d terms, served: 1 .. %d", K, FILTER_KMAX);
    CG_REQUIRE(J >= 1 && J <= FILTER_JMAX, "cheb_filter: J = %d filters, served: 1 .. %d", J, FILTER_JMAX);
    CG_REQUIRE(arm >= 0 && arm <= 2, "cheb_filter: arm = %d (0 automatic, 1 rolling, 2 stack)", arm);
    CG_REQUIRE(nplanes >= 1 && nplanes < (1 << 30), "cheb_filter: nplanes = %d, served: 1 .. 2^30 - 1", nplanes);
    CG_REQUIRE(g && x && coeff && y, "cheb_filter: NULL argument");
    CG_REQUIRE(workspace || K == 1, "cheb_filter: NULL workspace");
    const size_t slab = (size_t)nplanes * g->Mp;
    CG_REQUIRE(y + (size_t)J * slab <= x || x + slab <= y, "cheb_filter: y overlaps x");
    CG_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)workspace) & 15) == 0 && ((uintptr_t)coeff & 3) == 0,
               "cheb_filter: x, y and workspace must be 16-byte aligned");
    const int a = filter_arm(g, K, arm);
    if (a == 2 && !(g->lds_ok || g->ord_ok))
        return fail(CHEBGCN_EUNSUPPORTED, "cheb_filter: arm = 2 (stack) needs a graph with an on-chip or ordered image (M = %d)", g->M);
    hipStream_t stream = (hipStream_t)stream_;
    if (a == 2) return filter_stack(g, x, coeff, y, (float*)workspace, nplanes, K, J, stream);
    return filter_rolling(g, x, coeff, y, (float*)workspace, nplanes, K, J, stream);
}
