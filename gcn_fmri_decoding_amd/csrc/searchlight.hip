// Searchlight decoding with Gaussian naive Bayes (searchlight.searchlight): at every centre a cross-validated classifier sees only
// the centre's neighbourhood, and the centre gets its accuracy.
//
// The fit of naive Bayes is per-vertex moments and its decision a sum over the neighbourhood, so ONE fit per training set serves
// every centre.  A model is a training set (a (group, fold) pair within subjects, a fold across them); its test samples are
// contiguous columns of the vertex-major patterns Xt [M][Sp] (Sp = plane_stride(S)), because the caller sorts the samples by
// model.  Everything is float64 in the centred form (x - mu)^2 / (2 sigma^2): BOLD has mean / sd of 1e2 .. 1e4, and the expanded
// quadratic a x^2 + b x + d cancels by (mean / sd)^2.
//
//   searchlight_spread  thread (model, vertex): the variance of the whole training set at that vertex (two passes over the
//                       model's list), whose maximum over the vertices -- a reduction of the caller's -- scales the smoothing.
//   searchlight_fit     thread (model, vertex): per class the two-pass moments over the class's training list in list order, then
//                       mu, h = 1 / (2 sigma^2) and lg = log(2 pi sigma^2) / 2 with the smoothing added (pooled: one sigma^2 for
//                       all classes).  The tables are contiguous per (model, vertex): par [NM][M][NC][2] = (mu, h), lg [NM][M][NC],
//                       NC the class bucket, classes beyond C zero.  Cost S x folds x M: not the hot path, written plainly.
//   searchlight_base    thread (model, centre, class): base = log prior - sum_v lg over the centre's row in ascending entry order:
//                       formed once per (model, class, centre), not per sample.
//   searchlight_score<NC>  the hot path.  Workgroup = 4 waves, one centre each; the 64 lanes of a wave are 64 consecutive test
//                       samples of one model (with up to 8 classes: two runs of 64), so a neighbour's row of Xt is read
//                       coalesced.  A lane keeps NC float64 accumulators per sample (2 NC VGPRs).  The neighbour list and the
//                       neighbour's (mu, h) pairs are the same for every lane: their addresses are functions of the block, the
//                       wave and the loop counter alone, so they come through the scalar cache and enter the arithmetic as scalar
//                       operands; two samples per lane halve the scalar bytes per term.  Per (neighbour, class):
//                       t = x - mu; acc = fma(t h, t, acc) -- one subtraction, one multiply, one fma, nothing that depends on tile,
//                       wave or batch.  Two (wide buckets: four) neighbours' loads are issued before the arithmetic of the
//                       first.  Then score = base - acc, the first maximal class, and sl_tally (searchlight_common.h):
//                       correct[group][label][centre] += 1 with int32 atomics, one per distinct (group, label) of the wave.
// No float atomics anywhere.  Nothing read from memory is an address or a trip count unchecked: list and row pointers are clamped
// into their arrays, sample and vertex numbers outside [0, S) / [0, M) are skipped, group and label numbers outside their ranges
// add nothing.
#include "searchlight_common.h"

namespace chebgcn {

#ifndef CG_SL_U
#define CG_SL_U 4
#endif
#ifndef CG_SL_V2
#define CG_SL_V2 2
#endif
#ifndef CG_SL_U2
#define CG_SL_U2 2
#endif
constexpr int SL_LANES = 64;                // lanes of a score wave
constexpr int SL_NW = 4;                    // waves of a score workgroup: one centre each
constexpr int SL_NARROW = 8;                // class buckets up to this one are narrow: a lane owns SL_V2 test samples, not one
constexpr int SL_V2 = CG_SL_V2;             // (measured at 8 classes: 0.88 ms with two samples per lane and two neighbours in
constexpr int SL_U2 = CG_SL_U2;             //  flight, 0.95 with two and four, 1.10 with one and four or eight: DESIGN 4.23)
constexpr int SL_U = CG_SL_U;               // neighbours of a wave in flight, wide buckets
constexpr int sl_v(int NC) { return NC <= SL_NARROW ? SL_V2 : 1; }
constexpr int sl_u(int NC) { return NC <= SL_NARROW ? SL_U2 : SL_U; }
constexpr int SL_T = 256;                   // threads of spread / fit / base

// the class bucket of C classes: the width of the parameter tables and the accumulators of the score kernel
static inline int sl_bucket(int C) { return C <= 2 ? 2 : C <= 4 ? 4 : C <= 8 ? 8 : C <= 16 ? 16 : 32; }

// Two-pass moments of row[list[i]], i ascending: cnt entries inside [0, S), their mean, and the sum of squared deviations from it
__device__ __forceinline__ void sl_moments(const float* __restrict__ row, const int32_t* __restrict__ list, int n, int S, int& cnt,
                                           double& mu, double& ss) {
    double s = 0.0;
    cnt = 0;
    for (int i = 0; i < n; ++i) {
        const int j = list[i];
        if ((unsigned)j >= (unsigned)S) continue;
        s = s + (double)row[j];
        ++cnt;
    }
    mu = cnt ? s / (double)cnt : 0.0;
    ss = 0.0;
    for (int i = 0; i < n; ++i) {
        const int j = list[i];
        if ((unsigned)j >= (unsigned)S) continue;
        const double d = (double)row[j] - mu;
        ss = fma(d, d, ss);
    }
}

// block (256 vertices, model blockIdx.y)
__global__ void __launch_bounds__(SL_T)
searchlight_spread_kernel(const float* __restrict__ Xt, int S, int Sp, int M, const int32_t* __restrict__ lptr,
                          const int32_t* __restrict__ lidx, int nidx, double* __restrict__ spread) {
    const int v = blockIdx.x * SL_T + threadIdx.x;
    const int m = blockIdx.y;
    if (v >= M) return;
    const int i0 = sl_clamp(lptr[m], 0, nidx), i1 = sl_clamp(lptr[m + 1], i0, nidx);
    int cnt;
    double mu, ss;
    sl_moments(Xt + (size_t)v * Sp, lidx + i0, i1 - i0, S, cnt, mu, ss);
    spread[(size_t)m * M + v] = cnt ? ss / (double)cnt : 0.0;
}

// block (256 vertices, model blockIdx.y)
__global__ void __launch_bounds__(SL_T)
searchlight_fit_kernel(const float* __restrict__ Xt, int S, int Sp, int M, const int32_t* __restrict__ cptr,
                       const int32_t* __restrict__ cidx, int nidx, int C, int NC, int pooled, const double* __restrict__ eps,
                       double* __restrict__ par, double* __restrict__ lg) {
    const int v = blockIdx.x * SL_T + threadIdx.x;
    const int m = blockIdx.y;
    if (v >= M) return;
    const float* row = Xt + (size_t)v * Sp;
    double* q = par + ((size_t)m * M + v) * (2 * NC);
    double* l = lg + ((size_t)m * M + v) * NC;
    double pss = 0.0;
    long long pn = 0;
    for (int c = 0; c < C; ++c) {
        const int i0 = sl_clamp(cptr[m * C + c], 0, nidx), i1 = sl_clamp(cptr[m * C + c + 1], i0, nidx);
        int cnt;
        double mu, ss;
        sl_moments(row, cidx + i0, i1 - i0, S, cnt, mu, ss);
        q[2 * c] = mu;
        q[2 * c + 1] = cnt ? ss / (double)cnt : -1.0;       // the variance, until the second loop; -1: a class without samples
        pss = pss + ss;
        pn += cnt;
    }
    const double pv = pn ? pss / (double)pn : 0.0;
    const double e = eps[m];
    for (int c = 0; c < NC; ++c) {
        double h = 0.0, g = 0.0;
        if (c < C && q[2 * c + 1] >= 0.0) {
            const double var = (pooled ? pv : q[2 * c + 1]) + e;
            if (var > 0.0) {
                h = 1.0 / (2.0 * var);
                g = 0.5 * log(6.283185307179586476925 * var);
            }
        } else {
            q[2 * c] = 0.0;
        }
        q[2 * c + 1] = h;
        l[c] = g;
    }
}

// thread (class fastest, centre of the batch), model blockIdx.y
__global__ void __launch_bounds__(SL_T)
searchlight_base_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx, int nnz, int u0, int Ub, int M, int NC,
                        const double* __restrict__ lg, const double* __restrict__ logprior, double* __restrict__ base) {
    const long long t = (long long)blockIdx.x * SL_T + threadIdx.x;
    const int m = blockIdx.y;
    if (t >= (long long)Ub * NC) return;
    const int c = (int)(t % NC), ub = (int)(t / NC);
    const int r0 = sl_clamp(rowptr[u0 + ub], 0, nnz), r1 = sl_clamp(rowptr[u0 + ub + 1], r0, nnz);
    const double* l = lg + (size_t)m * M * NC + c;
    double sum = 0.0;
    for (int j = r0; j < r1; ++j) {
        const int v = colidx[j];
        if ((unsigned)v >= (unsigned)M) continue;
        sum = sum + l[(size_t)v * NC];
    }
    base[((size_t)m * Ub + ub) * NC + c] = logprior[m * NC + c] - sum;
}

struct SlScore {
    const float* Xt;            // [M][Sp]
    const int32_t* rowptr;      // [U + 1]
    const int32_t* colidx;      // [nnz]
    const int32_t* tptr;        // [NM + 1] test samples of a model
    const double* par;          // [NM][M][NC][2]
    const double* base;         // [NM][Ub][NC]
    const int32_t* sgroup;      // [S]
    const int32_t* slabel;      // [S]
    const int32_t* sorig;       // [S]
    int32_t* correct;           // [G][C][U]
    double* scores;             // [S][C][U] or NULL
    uint8_t* predictions;       // [S][U] or NULL
    int S, Sp, M, nnz, U, u0, Ub, C, G;
};

// block (4 centres of the batch: one per wave; tile blockIdx.y of 64 V test samples; model blockIdx.z); U neighbours in flight
template <int NC, int V, int U>
__global__ void __launch_bounds__(SL_NW * SL_LANES)
searchlight_score_kernel(SlScore p) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int ub = blockIdx.x * SL_NW + w;
    const int m = blockIdx.z;
    if (ub >= p.Ub) return;
    const int t0 = sl_clamp(p.tptr[m], 0, p.S), t1 = sl_clamp(p.tptr[m + 1], t0, p.S);
    if ((long long)t0 + (long long)blockIdx.y * (SL_LANES * V) >= t1) return;
    const int sb = t0 + blockIdx.y * (SL_LANES * V);
    // sample k of a lane is sb + 64 k + lane; one beyond the model's samples reads the tile's first and is dropped
    int s[V];
    bool live[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        live[k] = t1 - sb > SL_LANES * k + lane;
        s[k] = live[k] ? sb + SL_LANES * k + lane : sb;
    }
    const int u = p.u0 + ub;
    const int r0 = sl_clamp(p.rowptr[u], 0, p.nnz), r1 = sl_clamp(p.rowptr[u + 1], r0, p.nnz);
    const double* par = p.par + (size_t)m * p.M * (2 * NC);

    double acc[V][NC];
#pragma unroll
    for (int k = 0; k < V; ++k)
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[k][c] = 0.0;
    // U neighbours' loads before the arithmetic of the first; an entry at or beyond r1 is read as entry r1 - 1 and never used
    for (int j = r0; j < r1; j += U) {
        int vv[U];
        float xx[U][V];
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int v = p.colidx[min(j + i, r1 - 1)];
            vv[i] = (unsigned)v < (unsigned)p.M ? v : -1;
        }
#pragma unroll
        for (int i = 0; i < U; ++i)
#pragma unroll
            for (int k = 0; k < V; ++k) xx[i][k] = p.Xt[(size_t)max(vv[i], 0) * p.Sp + s[k]];
#pragma unroll
        for (int i = 0; i < U; ++i) {
            if (j + i < r1 && vv[i] >= 0) {
                const double* q = par + (size_t)vv[i] * (2 * NC);
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const double mu = q[2 * c], h = q[2 * c + 1];
#pragma unroll
                    for (int k = 0; k < V; ++k) {
                        const double t = (double)xx[i][k] - mu;
                        acc[k][c] = fma(t * h, t, acc[k][c]);
                    }
                }
            }
        }
    }

    const double* b = p.base + ((size_t)m * p.Ub + ub) * NC;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        double best = 0.0;
        int pred = 0;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            acc[k][c] = b[c] - acc[k][c];
            if (c < p.C && (c == 0 || acc[k][c] > best)) {
                best = acc[k][c];
                pred = c;
            }
        }
        if (live[k]) {
            const size_t so = (size_t)sl_clamp(p.sorig[s[k]], 0, p.S - 1);
            if (p.scores) {
#pragma unroll
                for (int c = 0; c < NC; ++c)
                    if (c < p.C) p.scores[(so * p.C + c) * p.U + u] = acc[k][c];
            }
            if (p.predictions) p.predictions[so * p.U + u] = (uint8_t)pred;
        }
        const int g = p.sgroup[s[k]], y = p.slabel[s[k]];
        sl_tally(p.correct, live[k] && pred == y && (unsigned)g < (unsigned)p.G ? g * p.C + y : -1, p.U, u, lane);
    }
}

template <int NC>
static void sl_launch_score(const SlScore& p, int tmax, int NM, hipStream_t stream) {
    static char name[40];
    static const int named = snprintf(name, sizeof name, "searchlight_score_kernel<%d>", NC);
    (void)named;
    note_dispatch_more(name);
    constexpr int V = sl_v(NC);
    const dim3 grid((unsigned)((p.Ub + SL_NW - 1) / SL_NW), (unsigned)((tmax + SL_LANES * V - 1) / (SL_LANES * V)), (unsigned)NM);
    hipLaunchKernelGGL((searchlight_score_kernel<NC, V, sl_u(NC)>), grid, dim3(SL_NW * SL_LANES), 0, stream, p);
}

static inline bool sl_patterns_ok(int S, int M) { return S >= 1 && M >= 1 && S <= INT_MAX - 31; }

}  // namespace chebgcn

using namespace chebgcn;

extern "C" int chebgcn_searchlight_query(int what) {
    switch (what) {
        case 0: return SL_LANES;            // lanes of a score wave: a tile is this many test samples per sample of a lane
        case 1: return SL_NW;               // centres of a score workgroup
        case 2: return SL_U;                // neighbours in flight, wide class buckets
        case 3: return SL_CMAX;             // the largest number of classes
        case 4: return SL_T;                // threads (vertices) of a spread / fit workgroup
        case 5: return SL_NMAX;             // models of one call
        case 6: return SL_TILES;            // tiles of a model's test samples
        case 7: return SL_GMAX;             // groups
        case 8: return SL_NARROW;           // the widest narrow class bucket
        case 9: return SL_V2;               // test samples of a lane, narrow buckets (wide ones: 1)
        case 10: return SL_U2;              // neighbours in flight, narrow buckets
        default:
            if (what > 100 && what <= 100 + SL_CMAX) return sl_bucket(what - 100);     // the class bucket of what - 100 classes
            return -1;
    }
}

extern "C" int chebgcn_searchlight_spread(const float* Xt, int S, int M, const int32_t* list_ptr, const int32_t* list_idx, int nidx, int NM,
                                          double* spread, chebgcn_stream stream_) {
    CG_REQUIRE(Xt && list_ptr && list_idx && spread, "searchlight_spread: NULL argument");
    CG_REQUIRE(sl_patterns_ok(S, M) && nidx >= 1 && NM >= 1, "searchlight_spread: bad shape (S = %d, M = %d, %d listed samples, NM = %d)", S,
               M, nidx, NM);
    if (NM > SL_NMAX) return fail(CHEBGCN_EUNSUPPORTED, "searchlight_spread: NM = %d; served: NM <= %d", NM, SL_NMAX);
    CG_REQUIRE((((uintptr_t)Xt | (uintptr_t)list_ptr | (uintptr_t)list_idx) & 3) == 0 && ((uintptr_t)spread & 7) == 0,
               "searchlight_spread: unaligned argument");
    note_dispatch("searchlight_spread_kernel");
    hipLaunchKernelGGL(searchlight_spread_kernel, dim3((unsigned)((M + SL_T - 1) / SL_T), (unsigned)NM), dim3(SL_T), 0, (hipStream_t)stream_,
                       Xt, S, plane_stride(S), M, list_ptr, list_idx, nidx, spread);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_searchlight_fit(const float* Xt, int S, int M, const int32_t* class_ptr, const int32_t* class_idx, int nidx, int NM,
                                       int C, int pooled, const double* eps, double* par, double* lg, chebgcn_stream stream_) {
    CG_REQUIRE(Xt && class_ptr && class_idx && eps && par && lg, "searchlight_fit: NULL argument");
    CG_REQUIRE(sl_patterns_ok(S, M) && nidx >= 1 && NM >= 1 && C >= 2 && (pooled == 0 || pooled == 1),
               "searchlight_fit: bad shape (S = %d, M = %d, %d listed samples, NM = %d, C = %d, pooled = %d)", S, M, nidx, NM, C, pooled);
    if (NM > SL_NMAX || C > SL_CMAX)
        return fail(CHEBGCN_EUNSUPPORTED, "searchlight_fit: NM = %d, C = %d; served: NM <= %d, C <= %d", NM, C, SL_NMAX, SL_CMAX);
    CG_REQUIRE((((uintptr_t)Xt | (uintptr_t)class_ptr | (uintptr_t)class_idx) & 3) == 0 &&
                   (((uintptr_t)eps | (uintptr_t)par | (uintptr_t)lg) & 7) == 0,
               "searchlight_fit: unaligned argument");
    note_dispatch("searchlight_fit_kernel");
    hipLaunchKernelGGL(searchlight_fit_kernel, dim3((unsigned)((M + SL_T - 1) / SL_T), (unsigned)NM), dim3(SL_T), 0, (hipStream_t)stream_, Xt,
                       S, plane_stride(S), M, class_ptr, class_idx, nidx, C, sl_bucket(C), pooled, eps, par, lg);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_searchlight_score(const float* Xt, int S, int M, const int32_t* rowptr, const int32_t* colidx, int nnz, int U, int u0,
                                         int Ub, const int32_t* test_ptr, int tmax, int NM, int C, const double* par, const double* lg,
                                         const double* logprior, const int32_t* sgroup, const int32_t* slabel, const int32_t* sorig,
                                         int G, double* base, int32_t* correct, double* scores, uint8_t* predictions,
                                         chebgcn_stream stream_) {
    CG_REQUIRE(Xt && rowptr && colidx && test_ptr && par && lg && logprior && sgroup && slabel && sorig && base && correct,
               "searchlight_score: NULL argument");
    CG_REQUIRE(sl_patterns_ok(S, M) && nnz >= 1 && U >= 1 && u0 >= 0 && Ub >= 1 && u0 <= U - Ub && tmax >= 1 && tmax <= S && NM >= 1 &&
                   C >= 2 && G >= 1,
               "searchlight_score: bad shape (S = %d, M = %d, nnz = %d, U = %d, centres [%d, %d + %d), tmax = %d, NM = %d, C = %d, G = %d)",
               S, M, nnz, U, u0, u0, Ub, tmax, NM, C, G);
    const long long tiles = ((long long)tmax + SL_LANES - 1) / SL_LANES;
    if (NM > SL_NMAX || C > SL_CMAX || G > SL_GMAX || tiles > SL_TILES || (long long)Ub * SL_CMAX > INT_MAX)
        return fail(CHEBGCN_EUNSUPPORTED, "searchlight_score: NM = %d, C = %d, G = %d, tmax = %d, Ub = %d; served: NM <= %d, C <= %d, "
                    "G <= %d, tmax <= %d, Ub <= %d", NM, C, G, tmax, Ub, SL_NMAX, SL_CMAX, SL_GMAX, SL_TILES * SL_LANES, INT_MAX / SL_CMAX);
    CG_REQUIRE((((uintptr_t)Xt | (uintptr_t)rowptr | (uintptr_t)colidx | (uintptr_t)test_ptr | (uintptr_t)sgroup | (uintptr_t)slabel |
                 (uintptr_t)sorig | (uintptr_t)correct) & 3) == 0 &&
                   (((uintptr_t)par | (uintptr_t)lg | (uintptr_t)logprior | (uintptr_t)base | (uintptr_t)scores) & 7) == 0,
               "searchlight_score: unaligned argument");
    const int NC = sl_bucket(C);
    hipStream_t stream = (hipStream_t)stream_;
    note_dispatch("searchlight_base_kernel");
    hipLaunchKernelGGL(searchlight_base_kernel, dim3((unsigned)(((long long)Ub * NC + SL_T - 1) / SL_T), (unsigned)NM), dim3(SL_T), 0, stream,
                       rowptr, colidx, nnz, u0, Ub, M, NC, lg, logprior, base);
    const SlScore p{Xt, rowptr, colidx, test_ptr, par, base, sgroup, slabel, sorig, correct, scores, predictions,
                    S, plane_stride(S), M, nnz, U, u0, Ub, C, G};
    switch (NC) {
        case 2: sl_launch_score<2>(p, tmax, NM, stream); break;
        case 4: sl_launch_score<4>(p, tmax, NM, stream); break;
        case 8: sl_launch_score<8>(p, tmax, NM, stream); break;
        case 16: sl_launch_score<16>(p, tmax, NM, stream); break;
        default: sl_launch_score<32>(p, tmax, NM, stream); break;
    }
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}
