// Parcellation (parcellation.Parcellation): a vertex-level run [T][V] reduced to the R regions of an atlas, and the inverse gather.
//
//   parcellate:  out[t][r] = (sum_j x[t][idx[j]]) / n_r,  j over the members ptr[r] .. ptr[r + 1) of region r in ASCENDING j (the
//                members of a region ascend in V): float32, acc = 0, acc = acc + x one member after the other, ONE rounded division
//                at the end.  With weights: acc = acc + w[v] * x (the product rounded on its own, never an fma), the denominator
//                den = den + w[v] in the same order, out = acc / den.  mode SUM leaves the division out.  The order is a function
//                of (ptr, idx) alone: not of T, the row tile, the grid, the chunk of V a workgroup holds or the pass a region
//                falls in.  No float atomics.
//   expand:      out[b][v] = maps[b][region_of[v]], `fill` where region_of[v] is outside [0, R).
//
// Rows are contiguous over V and a region's members are scattered in it, so a workgroup owns ROWS rows and sweeps V in chunks of
// PC_TILE / ROWS vertices: the chunk goes HBM -> registers -> LDS in aligned 16-byte pieces (a row starts wherever t * ldx puts it:
// every row has its own shift of 0..3 floats into the LDS image, and only the pieces that straddle an end of the row are loaded
// element by element), then thread `tid` adds the chunk's members of ITS regions (p0 + tid, p0 + PC_T + tid) from LDS into
// registers.  A thread walks its member list with a cursor: the indices come four at a time, one batch ahead of the adds.
//
// Why one LDS buffer and no prefetch of the next chunk: the member indices are vector loads as well, and the wave's load counter
// retires in order -- the first index a thread waits for would wait for the whole prefetched chunk behind which it was issued.
// The overlap of HBM latency and adds comes from the other workgroups of the CU instead (16.4 KB of LDS each: eight fit).
#include <limits.h>

#include "common.h"

namespace chebgcn {

constexpr int PC_T = 256;               // threads
constexpr int PC_TILE = 4096;           // floats of x in LDS per workgroup: ROWS rows of PC_TILE / ROWS vertices
constexpr int PC_RPT = 2;               // regions a thread accumulates per pass
constexpr int PC_PASS = PC_T * PC_RPT;  // regions of one pass over V; R beyond it sweeps V again
constexpr int PC_ROWS = 4;              // the wide arm's row tile (the narrow arm: one row, more workgroups)
constexpr int PC_WIDE_T = 4096;         // rows from which the wide arm runs
constexpr int PC_GRID = 16384;          // workgroups at most: a workgroup loops over its row tiles
constexpr int PC_BATCH = 4;             // member indices in flight per thread and region

constexpr int PE_T = 256;               // threads of the expand kernel, 4 vertices each
constexpr int PE_GRID_Y = 1024;         // map rows of the grid at most: a workgroup loops over b

// the aligned 16 bytes at xa + s0 (s0 = 4q: shifted coordinate, vertex = s0 - sh); elements outside [0, V) are not read
__device__ __forceinline__ float4 load_piece(const float* __restrict__ xa, int sh, int s0, int V) {
    const int v0 = s0 - sh;
    if (v0 >= 0 && v0 + 3 < V) return *reinterpret_cast<const float4*>(xa + s0);
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (v0 + 3 < 0 || v0 >= V) return r;
    if (v0 >= 0) r.x = xa[s0];
    if (v0 + 1 >= 0 && v0 + 1 < V) r.y = xa[s0 + 1];
    if (v0 + 2 >= 0 && v0 + 2 < V) r.z = xa[s0 + 2];
    if (v0 + 3 < V) r.w = xa[s0 + 3];
    return r;
}

// the members of one region inside the chunk [c0, c0 + VC): cursor j, next unconsumed member vh (INT_MAX: none left)
template <int ROWS, bool W, int LD, int VC>
__device__ __forceinline__ void add_members(const float* tile, const int (&sh)[ROWS], const int32_t* __restrict__ idx,
                                            const float* __restrict__ w, int V, int c0, int& j, int je, int& vh,
                                            float (&acc)[ROWS], float& den) {
    const int cend = c0 + VC;
    if (vh >= cend) return;
    int nb[PC_BATCH];
#pragma unroll
    for (int k = 0; k < PC_BATCH; ++k) nb[k] = j + k < je ? idx[j + k] : INT_MAX;
    for (;;) {
        int vb[PC_BATCH];
        float wb[PC_BATCH];
#pragma unroll
        for (int k = 0; k < PC_BATCH; ++k) vb[k] = nb[k];
#pragma unroll
        for (int k = 0; k < PC_BATCH; ++k) nb[k] = j + PC_BATCH + k < je ? idx[j + PC_BATCH + k] : INT_MAX;
        if (W) {
#pragma unroll
            for (int k = 0; k < PC_BATCH; ++k) wb[k] = (vb[k] < cend && (unsigned)vb[k] < (unsigned)V) ? w[vb[k]] : 0.f;
        }
        bool more = true;
#pragma unroll
        for (int k = 0; k < PC_BATCH; ++k) {
            if (more) {
                if (vb[k] < cend) {
                    const unsigned off = (unsigned)(vb[k] - c0);
                    if (off < (unsigned)VC) {       // (a list that does not ascend is skipped, never an address)
#pragma unroll
                        for (int i = 0; i < ROWS; ++i) {
                            const float xv = tile[i * LD + (int)off + sh[i]];
                            acc[i] = __fadd_rn(acc[i], W ? __fmul_rn(wb[k], xv) : xv);
                        }
                        if (W) den = __fadd_rn(den, wb[k]);
                    }
                    ++j;
                } else {
                    vh = vb[k];
                    more = false;
                }
            }
        }
        if (!more) break;
    }
}

// block: row tiles tb = blockIdx.x, + gridDim.x, ...
template <int ROWS, bool W>
__global__ void __launch_bounds__(PC_T)
parcellate_kernel(const float* __restrict__ x, long long ldx, const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                  int nnz, const float* __restrict__ w, float* __restrict__ out, long long ldo, long long T, int V, int R,
                  int mode) {
    constexpr int VC = PC_TILE / ROWS, LD = VC + 4, NQ = VC / 4, U = PC_TILE / 4 / PC_T, UR = U / ROWS;
    static_assert(U % ROWS == 0 && NQ == UR * PC_T, "a thread's pieces of a chunk belong to rows known at compile time");
    __shared__ float4 tile4[ROWS * LD / 4];
    const float* tile = reinterpret_cast<const float*>(tile4);
    const int tid = threadIdx.x;
    const long long ntiles = (T + ROWS - 1) / ROWS;
    const int nchunks = (V + VC - 1) / VC;
    for (long long tb = blockIdx.x; tb < ntiles; tb += gridDim.x) {
        const long long t0 = tb * ROWS;
        const float* xa[ROWS];          // the row's start rounded down to 16 bytes, and how many floats that took
        int sh[ROWS];
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const long long t = t0 + i < T ? t0 + i : T - 1;
            const float* xr = x + t * ldx;
            sh[i] = (int)(((uintptr_t)xr >> 2) & 3);
            xa[i] = xr - sh[i];
        }
        for (int p0 = 0; p0 < R; p0 += PC_PASS) {
            float acc[PC_RPT][ROWS], den[PC_RPT], cnt[PC_RPT];
            int j[PC_RPT], je[PC_RPT], vh[PC_RPT];
#pragma unroll
            for (int s = 0; s < PC_RPT; ++s) {
                const int r = p0 + s * PC_T + tid;
                j[s] = je[s] = 0;
                if (r < R) {
                    j[s] = min(max(ptr[r], 0), nnz);
                    je[s] = min(max(ptr[r + 1], j[s]), nnz);
                }
                cnt[s] = (float)(je[s] - j[s]);
                vh[s] = j[s] < je[s] ? idx[j[s]] : INT_MAX;
                den[s] = 0.f;
#pragma unroll
                for (int i = 0; i < ROWS; ++i) acc[s][i] = 0.f;
            }
            for (int c = 0; c < nchunks; ++c) {
                const int c0 = c * VC;
                float4 st[U], ex = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int u = 0; u < U; ++u)     // piece u of this thread: row u / UR, float4 (u % UR) * PC_T + tid of the row
                    st[u] = load_piece(xa[u / UR], sh[u / UR], c0 + 4 * ((u % UR) * PC_T + tid), V);
#pragma unroll
                for (int i = 0; i < ROWS; ++i)  // the piece a shifted row needs behind its last full one
                    if (tid == i) ex = load_piece(xa[i], sh[i], c0 + VC, V);
                __syncthreads();                // every thread is done with the chunk before
#pragma unroll
                for (int u = 0; u < U; ++u) tile4[(u / UR) * (LD / 4) + (u % UR) * PC_T + tid] = st[u];
                if (tid < ROWS) tile4[tid * (LD / 4) + NQ] = ex;
                __syncthreads();
#pragma unroll
                for (int s = 0; s < PC_RPT; ++s)
                    add_members<ROWS, W, LD, VC>(tile, sh, idx, w, V, c0, j[s], je[s], vh[s], acc[s], den[s]);
            }
#pragma unroll
            for (int s = 0; s < PC_RPT; ++s) {
                const int r = p0 + s * PC_T + tid;
                if (r < R) {
                    const float d = W ? den[s] : cnt[s];
#pragma unroll
                    for (int i = 0; i < ROWS; ++i)
                        if (t0 + i < T)
                            out[(t0 + i) * ldo + r] = mode == CHEBGCN_PARCEL_MEAN ? __fdiv_rn(acc[s][i], d) : acc[s][i];
                }
            }
        }
    }
}

// block (piece of 4 * PE_T vertices, map rows b = blockIdx.y, + gridDim.y, ...)
__global__ void __launch_bounds__(PE_T)
parcel_expand_kernel(const float* __restrict__ maps, const int32_t* __restrict__ region_of, float* __restrict__ out, int B, int R,
                     int V, float fill) {
    const int v0 = 4 * (blockIdx.x * PE_T + threadIdx.x);
    if (v0 >= V) return;
    const bool full = v0 + 3 < V;
    int r[4] = {-1, -1, -1, -1};
    if (full) {
        const int4 q = *reinterpret_cast<const int4*>(region_of + v0);     // region_of is 16-byte aligned (checked)
        r[0] = q.x; r[1] = q.y; r[2] = q.z; r[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (v0 + e < V) r[e] = region_of[v0 + e];
    }
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const float* m = maps + (long long)b * R;
        float val[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) val[e] = (unsigned)r[e] < (unsigned)R ? m[r[e]] : fill;
        float* dst = out + (long long)b * V + v0;
        if (full && ((uintptr_t)dst & 15) == 0) {
            *reinterpret_cast<float4*>(dst) = make_float4(val[0], val[1], val[2], val[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (v0 + e < V) dst[e] = val[e];
        }
    }
}

}  // namespace chebgcn

using namespace chebgcn;

extern "C" int chebgcn_parcellate_query(int what) {
    switch (what) {
        case 0: return PC_TILE;             // floats of a chunk: PC_TILE / row tile vertices of every row
        case 1: return PC_ROWS;             // row tile of the wide arm (the narrow arm's is 1)
        case 2: return PC_WIDE_T;           // rows from which the wide arm runs
        case 3: return PC_PASS;             // regions a workgroup accumulates per pass over V
        case 4: return PC_GRID;             // workgroups of a parcellate launch at most
        case 5: return PE_GRID_Y;           // map rows of an expand grid at most
        case 6: return 4;                   // vertices per thread of the expand kernel
        default: return -1;
    }
}

extern "C" int chebgcn_parcellate(const float* x, int64_t ldx, const int32_t* ptr, const int32_t* idx, int64_t nnz, const float* w,
                                  float* out, int64_t ldo, int64_t T, int V, int R, int mode, chebgcn_stream stream_) {
    CG_REQUIRE(x && ptr && idx && out, "parcellate: NULL argument");
    CG_REQUIRE(T >= 1 && V >= 1 && R >= 1, "parcellate: bad shape (T = %lld, V = %d, R = %d)", (long long)T, V, R);
    CG_REQUIRE(V <= (1 << 30), "parcellate: V = %d vertices, at most 2^30", V);
    CG_REQUIRE(R <= 65535, "parcellate: R = %d regions, at most 65535", R);
    CG_REQUIRE(ldx >= V, "parcellate: ldx = %lld is less than V = %d", (long long)ldx, V);
    CG_REQUIRE(ldo >= R, "parcellate: ldo = %lld is less than R = %d", (long long)ldo, R);
    CG_REQUIRE(nnz >= 0 && nnz <= V, "parcellate: nnz = %lld members of %d vertices (every vertex at most once)", (long long)nnz, V);
    CG_REQUIRE(mode == CHEBGCN_PARCEL_MEAN || mode == CHEBGCN_PARCEL_SUM, "parcellate: unknown mode %d", mode);
    CG_REQUIRE((((uintptr_t)x | (uintptr_t)out | (uintptr_t)w) & 3) == 0, "parcellate: x, w and out must be 4-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    const bool wide = T >= PC_WIDE_T;
    const int64_t ntiles = wide ? (T + PC_ROWS - 1) / PC_ROWS : T;
    const dim3 grid((unsigned)(ntiles < PC_GRID ? ntiles : PC_GRID));
#define CG_PARCELLATE(ROWS, W, NAME)                                                                                             \
    do {                                                                                                                         \
        note_dispatch(NAME);                                                                                                     \
        hipLaunchKernelGGL((parcellate_kernel<ROWS, W>), grid, dim3(PC_T), 0, stream, x, (long long)ldx, ptr, idx, (int)nnz, w,  \
                           out, (long long)ldo, (long long)T, V, R, mode);                                                       \
    } while (0)
    if (wide) {
        if (w) CG_PARCELLATE(PC_ROWS, true, "parcellate_kernel<rows4, weighted>");
        else CG_PARCELLATE(PC_ROWS, false, "parcellate_kernel<rows4, plain>");
    } else {
        if (w) CG_PARCELLATE(1, true, "parcellate_kernel<rows1, weighted>");
        else CG_PARCELLATE(1, false, "parcellate_kernel<rows1, plain>");
    }
#undef CG_PARCELLATE
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_parcel_expand(const float* maps, const int32_t* region_of, float* out, int64_t B, int R, int V, float fill,
                                     chebgcn_stream stream_) {
    CG_REQUIRE(maps && region_of && out, "parcel_expand: NULL argument");
    CG_REQUIRE(B >= 1 && B <= 0x7fffffffLL && V >= 1 && R >= 1, "parcel_expand: bad shape (B = %lld, R = %d, V = %d)", (long long)B,
               R, V);
    CG_REQUIRE(V <= (1 << 30), "parcel_expand: V = %d vertices, at most 2^30", V);
    CG_REQUIRE(R <= 65535, "parcel_expand: R = %d regions, at most 65535", R);
    CG_REQUIRE(((uintptr_t)region_of & 15) == 0 && (((uintptr_t)maps | (uintptr_t)out) & 3) == 0,
               "parcel_expand: region_of must be 16-byte aligned, maps and out 4-byte aligned");
    const dim3 grid((unsigned)((V + 4 * PE_T - 1) / (4 * PE_T)), (unsigned)(B < PE_GRID_Y ? B : PE_GRID_Y));
    note_dispatch("parcel_expand_kernel");
    hipLaunchKernelGGL(parcel_expand_kernel, grid, dim3(PE_T), 0, (hipStream_t)stream_, maps, region_of, out, (int)B, R, V, fill);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}
