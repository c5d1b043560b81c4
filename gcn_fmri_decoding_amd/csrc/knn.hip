// kNN brain graphs on the device (graph.knn_device / graph.connectivity_graph): the k nearest neighbours of every vertex from
// feature-major planes feat[D][Np], without ever forming the N x N distance matrix, and the per-run normalisation that turns a
// staged series into the operand of a mean-correlation Gram matrix.
//
//   prep      per vertex, float64 sums in ascending d: mean, centred norm, inverse norm; for cosine / correlation a normalised
//             copy Q[d][i] = (feat[d][i] - mu_i) / |.|_i, so that the similarity is the plain Gram matrix of Q (a zero-norm or
//             constant row becomes a zero row: similarity 0 to everything, never NaN); for euclidean  sq_i = |feat_i|^2.
//   select    every query keeps its KC = min(k + KNN_SLACK, N - 1) best candidates under a float32 KEY, in sorted lists that
//             live in LDS, one list per lane, guarded by the list's worst kept key (a candidate that does not beat it costs one
//             compare).  Two arms:
//               direct (D <= 8)  a thread per query, candidate tiles through LDS, key = sum_d (a - b)^2 by differences
//                                (euclidean) or -sum_d a b (cosine / correlation on Q), an fmaf chain in ascending d;
//               gram   (D > 8)   a wave owns 32 queries (the B operand of v_mfma_f32_32x32x2_f32: accumulator COLUMN = lane =
//                                query) and sweeps blocks of 128 candidates (the A operand: one 16-byte load along the vertex
//                                axis per k-step feeds four 32 x 32 tiles, row r of tile c = candidate c0 + 4 r + c), so a lane's
//                                64 accumulators are 64 candidates of its own query.  key = -(G_ij - sq_j / 2) for euclidean
//                                (one more matrix step with the operand pair (sq_j, -1/2): monotone in the squared distance
//                                for a fixed query), -G_ij otherwise.
//             Where the query blocks alone give fewer workgroups than the chip has CUs, the candidate range is split over
//             gridDim.y and every split writes its own partial lists.
//   merge     one wave per query: the partial lists (splits, and the two lane halves of the gram arm) are joined in a fixed
//             order into the KC best keys, the distance of each of those KC pairs is RECOMPUTED from the features by direct
//             differences / products with float64 accumulators in ascending d, and the k smallest (distance, index) are
//             written in ascending order.  The numbers returned are never the cancelling Gram form.
//
// No float atomics; every sum has a fixed order; lists are ordered by (key, index) and do not depend on arrival order: two
// calls give bit-identical outputs.  The slack argument (why a true neighbour survives the float32 selection) is DESIGN 4.12.
#include "common.h"

namespace chebgcn {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int KNN_T = 256;              // threads of every kernel here
constexpr int KNN_KMAX = 32;
constexpr int KNN_SLACK = 8;            // candidates kept beyond k by the float32 selection
constexpr int KNN_DSMALL = 8;           // direct arm up to this many features
constexpr int KNN_QB = 128;             // gram arm: queries of a workgroup (32 per wave)
constexpr int KNN_CB = 128;             // gram arm: candidates of one block (four 32 x 32 tiles)
constexpr int KNN_MAXSPLIT = 8;         // most pieces of the candidate range (partial lists per query: 8 direct, 16 gram)
constexpr int KNN_NONE = 0x7fffffff;    // index of an empty list entry (key +inf)

static inline int knn_kc(int N, int k) { return min(k + KNN_SLACK, N - 1); }

// ------------------------------------------------------------------------------------------------------------------
// prep / series_normalise: one thread per (vertex, run); float64 sums in ascending row order
// ------------------------------------------------------------------------------------------------------------------
// rows [t0, t1) of in[.][Mp].  centre: subtract the mean; returns the sum of squares of the (centred) values
__device__ __forceinline__ double column_stats(const float* __restrict__ in, long long t0, long long t1, int Mp, int m,
                                               bool centre, double* mu_out) {
    double mu = 0.0;
    if (centre) {
        double s = 0.0;
        for (long long t = t0; t < t1; ++t) s += (double)in[t * Mp + m];
        mu = s / (double)(t1 - t0);
    }
    double ss = 0.0;
    for (long long t = t0; t < t1; ++t) {
        const double d = (double)in[t * Mp + m] - mu;
        ss = fma(d, d, ss);
    }
    *mu_out = mu;
    return ss;
}

// block (256 vertices, run r): out[t][m] = (in[t][m] - mean) / norm * scale inside the run, a constant vertex and the pad 0
__global__ void __launch_bounds__(KNN_T)
series_normalise_kernel(const float* __restrict__ in, const long long* __restrict__ offs, int M, int Mp, float scale,
                        float* __restrict__ out) {
    const int m = blockIdx.x * KNN_T + threadIdx.x;
    if (m >= Mp) return;
    const long long t0 = offs[blockIdx.y], t1 = offs[blockIdx.y + 1];
    double mu = 0.0, inv = 0.0;
    if (m < M) {
        const double ss = column_stats(in, t0, t1, Mp, m, true, &mu);
        inv = ss > 0.0 ? (double)scale / sqrt(ss) : 0.0;
    }
    for (long long t = t0; t < t1; ++t) out[t * Mp + m] = m < M ? (float)(((double)in[t * Mp + m] - mu) * inv) : 0.f;
}

// thread per vertex i < Np: mu / inv (float64), sq (float32) and, for cosine / correlation, the normalised copy Q
__global__ void __launch_bounds__(KNN_T)
knn_prep_kernel(const float* __restrict__ feat, int N, int Np, int D, int metric, double* __restrict__ mu_out,
                double* __restrict__ inv_out, float* __restrict__ sq_out, float* __restrict__ Q) {
    const int i = blockIdx.x * KNN_T + threadIdx.x;
    if (i >= Np) return;
    double mu = 0.0, inv = 0.0, ss = 0.0;
    if (i < N) {
        if (metric == CHEBGCN_KNN_DOT) inv = 1.0;
        else {
            ss = column_stats(feat, 0, D, Np, i, metric == CHEBGCN_KNN_CORRELATION, &mu);
            inv = ss > 0.0 ? 1.0 / sqrt(ss) : 0.0;
        }
    }
    mu_out[i] = mu;
    inv_out[i] = inv;
    sq_out[i] = (float)ss;
    if (metric == CHEBGCN_KNN_COSINE || metric == CHEBGCN_KNN_CORRELATION)
        for (int d = 0; d < D; ++d) Q[(size_t)d * Np + i] = i < N ? (float)(((double)feat[(size_t)d * Np + i] - mu) * inv) : 0.f;
}

// ------------------------------------------------------------------------------------------------------------------
// the per-lane candidate list: KC entries sorted ascending by (key, index), entry c of thread t at [c * KNN_T + t]
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void list_offer(float* __restrict__ lkey, int* __restrict__ lidx, int kc, int t, float v, int cand,
                                           float& wk, int& wi) {
    if (!(v < wk || (v == wk && cand < wi))) return;
    int p = kc - 1;
    while (p > 0) {
        const float pk = lkey[(p - 1) * KNN_T + t];
        const int pi = lidx[(p - 1) * KNN_T + t];
        if (pk < v || (pk == v && pi < cand)) break;
        lkey[p * KNN_T + t] = pk;
        lidx[p * KNN_T + t] = pi;
        --p;
    }
    lkey[p * KNN_T + t] = v;
    lidx[p * KNN_T + t] = cand;
    wk = lkey[(kc - 1) * KNN_T + t];
    wi = lidx[(kc - 1) * KNN_T + t];
}

__device__ __forceinline__ void list_store(const float* __restrict__ lkey, const int* __restrict__ lidx, int kc, int t,
                                           float* __restrict__ pkey, int* __restrict__ pidx, size_t base) {
    for (int c = 0; c < kc; ++c) {
        pkey[base + c] = lkey[c * KNN_T + t];
        pidx[base + c] = lidx[c * KNN_T + t];
    }
}

// ------------------------------------------------------------------------------------------------------------------
// direct arm: block (256 queries, split s); list p = s of query i at part[(i * P + p) * kc]
// ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(KNN_T)
knn_direct_kernel(const float* __restrict__ Q, int N, int Np, int D, int kc, int cps, int euclid, int P,
                  float* __restrict__ pkey, int* __restrict__ pidx) {
    extern __shared__ float smem[];
    float* lkey = smem;
    int* lidx = reinterpret_cast<int*>(smem + kc * KNN_T);
    float* tile = smem + 2 * kc * KNN_T;                  // [KNN_DSMALL][KNN_T]
    const int t = threadIdx.x;
    const int qi = blockIdx.x * KNN_T + t;
    const int qa = min(qi, Np - 1);
    float x[KNN_DSMALL];
#pragma unroll
    for (int d = 0; d < KNN_DSMALL; ++d) x[d] = d < D ? Q[(size_t)d * Np + qa] : 0.f;
    for (int c = 0; c < kc; ++c) {
        lkey[c * KNN_T + t] = __builtin_inff();
        lidx[c * KNN_T + t] = KNN_NONE;
    }
    float wk = __builtin_inff();
    int wi = KNN_NONE;
    const int cbeg = blockIdx.y * cps, cend = min(N, cbeg + cps);
    for (int c0 = cbeg; c0 < cend; c0 += KNN_T) {
        __syncthreads();
#pragma unroll
        for (int d = 0; d < KNN_DSMALL; ++d)
            if (d < D) tile[d * KNN_T + t] = Q[(size_t)d * Np + min(c0 + t, Np - 1)];
        __syncthreads();
        const int n = min(KNN_T, cend - c0);
        if (qi < N) {
            for (int j = 0; j < n; ++j) {
                float v = 0.f;
#pragma unroll
                for (int d = 0; d < KNN_DSMALL; ++d) {
                    if (d < D) {
                        const float y = tile[d * KNN_T + j];
                        if (euclid) {
                            const float df = x[d] - y;
                            v = fmaf(df, df, v);
                        } else {
                            v = fmaf(x[d], y, v);
                        }
                    }
                }
                if (!euclid) v = -v;
                if (v <= wk && c0 + j != qi) list_offer(lkey, lidx, kc, t, v, c0 + j, wk, wi);
            }
        }
    }
    if (qi < N) list_store(lkey, lidx, kc, t, pkey, pidx, ((size_t)qi * P + blockIdx.y) * kc);
}

// ------------------------------------------------------------------------------------------------------------------
// gram arm: block (128 queries, split s); lane (j, h) of wave w keeps the list p = 2 s + h of query 128 bx + 32 w + j
// ------------------------------------------------------------------------------------------------------------------
struct GramFrag {
    float4 a[4];
    float b[4];
};

// four matrix steps = eight features from d0 on: step u takes feature d0 + 2 u + h from lane half h for both operands.
// Loads are unconditional at clamped addresses and masked afterwards (features beyond D, candidates beyond the plane).
__device__ __forceinline__ void gram_load(GramFrag& f, const float* __restrict__ Q, int Np, int D, int d0, int h, int ca, bool cin,
                                          int qa) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int dd = d0 + 2 * u + h;
        const bool ok = dd < D;
        const float* row = Q + (size_t)min(dd, D - 1) * Np;
        const float4 a = *reinterpret_cast<const float4*>(row + ca);
        const float b = row[qa];
        const bool oka = ok && cin;
        f.a[u] = make_float4(oka ? a.x : 0.f, oka ? a.y : 0.f, oka ? a.z : 0.f, oka ? a.w : 0.f);
        f.b[u] = ok ? b : 0.f;
    }
}

__global__ void __launch_bounds__(KNN_T)
knn_gram_kernel(const float* __restrict__ Q, const float* __restrict__ sq, int N, int Np, int D, int kc, int cbps, int euclid,
                int P, float* __restrict__ pkey, int* __restrict__ pidx) {
    extern __shared__ float smem[];
    float* lkey = smem;
    int* lidx = reinterpret_cast<int*>(smem + kc * KNN_T);
    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int i = lane & 31, h = lane >> 5;
    const int q0 = blockIdx.x * KNN_QB + wave * 32;
    if (q0 >= N) return;                                  // the whole wave (no barrier below)
    const int qi = q0 + i;                                // < Np: q0 and Np are multiples of 32
    for (int c = 0; c < kc; ++c) {
        lkey[c * KNN_T + t] = __builtin_inff();
        lidx[c * KNN_T + t] = KNN_NONE;
    }
    float wk = __builtin_inff();
    int wi = KNN_NONE;
    const int ncb = (N + KNN_CB - 1) / KNN_CB;
    const int cb0 = blockIdx.y * cbps, cb1 = min(ncb, cb0 + cbps);
    for (int cb = cb0; cb < cb1; ++cb) {
        const int c0 = cb * KNN_CB;
        const bool cin = c0 + 4 * i < Np;                 // Np is a multiple of 4: a 16-byte piece is inside or outside
        const int ca = min(c0 + 4 * i, Np - 4);
        f32x16 acc[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[c][q] = 0.f;
        GramFrag cur, nxt;
        gram_load(cur, Q, Np, D, 0, h, ca, cin, qi);
        for (int d0 = 0; d0 < D; d0 += 8) {
            gram_load(nxt, Q, Np, D, min(d0 + 8, D - 1), h, ca, cin, qi);      // the last turn's prefetch is not used
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a[u].x, cur.b[u], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a[u].y, cur.b[u], acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a[u].z, cur.b[u], acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a[u].w, cur.b[u], acc[3], 0, 0, 0);
            }
            cur = nxt;
        }
        if (euclid) {                                     // one more step: G_ij - sq_j / 2 (lane half 0 carries it, half 1 zero)
            const float4 s4 = *reinterpret_cast<const float4*>(sq + ca);
            const bool on = cin && h == 0;
            const float b = h == 0 ? -0.5f : 0.f;
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(on ? s4.x : 0.f, b, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(on ? s4.y : 0.f, b, acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(on ? s4.z : 0.f, b, acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(on ? s4.w : 0.f, b, acc[3], 0, 0, 0);
        }
        // accumulator q of tile c in lane (i, h): query q0 + i against candidate c0 + 4 ((q & 3) + 8 (q >> 2) + 4 h) + c
        if (qi < N) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float best = -acc[c][0];
#pragma unroll
                for (int q = 1; q < 16; ++q) best = fminf(best, -acc[c][q]);
                if (best <= wk) {
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int cand = c0 + 4 * ((q & 3) + 8 * (q >> 2) + 4 * h) + c;
                        const float v = -acc[c][q];
                        if (v <= wk && cand < N && cand != qi) list_offer(lkey, lidx, kc, t, v, cand, wk, wi);
                    }
                }
            }
        }
    }
    if (qi < N) list_store(lkey, lidx, kc, t, pkey, pidx, ((size_t)qi * P + 2 * blockIdx.y + h) * kc);
}

// ------------------------------------------------------------------------------------------------------------------
// merge + refine: wave per query
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool key_less(double a, int ia, double b, int ib) { return a < b || (a == b && ia < ib); }

__global__ void __launch_bounds__(KNN_T)
knn_merge_refine_kernel(const float* __restrict__ feat, const double* __restrict__ mu, const double* __restrict__ inv,
                        const float* __restrict__ pkey, const int* __restrict__ pidx, int N, int Np, int D, int k, int kc, int P,
                        int metric, float* __restrict__ dist_out, int* __restrict__ idx_out) {
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * (KNN_T / 64) + (threadIdx.x >> 6);
    if (qi >= N) return;                                  // the whole wave
    // 1. the kc smallest (key, index) of the P sorted lists: lane p < P walks list p; the winner of round r goes to lane r
    const size_t base = (size_t)qi * P * kc;
    int pos = 0, mine = KNN_NONE;
    for (int r = 0; r < kc; ++r) {
        float hk = __builtin_inff();
        int hi = KNN_NONE;
        if (lane < P && pos < kc) {
            hk = pkey[base + (size_t)lane * kc + pos];
            hi = pidx[base + (size_t)lane * kc + pos];
        }
        float bk = hk;
        int bi = hi;
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const float ok = __shfl_xor(bk, s);
            const int oi = __shfl_xor(bi, s);
            if (ok < bk || (ok == bk && oi < bi)) { bk = ok; bi = oi; }
        }
        if (hi == bi && hi != KNN_NONE) ++pos;            // a candidate sits in exactly one list
        if (lane == r) mine = bi;
    }
    // 2. the distance of (qi, mine) from the features themselves, float64, ascending d
    const bool live = lane < kc && mine != KNN_NONE;
    const int j = live ? mine : qi;
    double acc = 0.0;
    if (metric == CHEBGCN_KNN_EUCLIDEAN) {
        for (int d = 0; d < D; ++d) {
            const double df = (double)feat[(size_t)d * Np + qi] - (double)feat[(size_t)d * Np + j];
            acc = fma(df, df, acc);
        }
        acc = sqrt(acc);
    } else {
        const double mi = mu[qi], mj = mu[j];
        for (int d = 0; d < D; ++d)
            acc = fma((double)feat[(size_t)d * Np + qi] - mi, (double)feat[(size_t)d * Np + j] - mj, acc);
        acc *= inv[qi] * inv[j];
        if (metric != CHEBGCN_KNN_DOT) acc = fmin(1.0, fmax(-1.0, acc));
        acc = 1.0 - acc;
    }
    // 3. rank by (distance, index); the k first leave in ascending order
    int rank = 0;
    for (int c = 0; c < kc; ++c) {
        const double ov = __shfl(acc, c);
        const int oi = __shfl(mine, c);
        rank += (oi != KNN_NONE && key_less(ov, oi, acc, mine)) ? 1 : 0;
    }
    if (live && rank < k) {
        dist_out[(size_t)qi * k + rank] = (float)acc;
        idx_out[(size_t)qi * k + rank] = mine;
    }
}

struct KnnPlan {
    bool direct;
    int kc, nqb, nsplit, per, P;         // per: candidates (direct) or candidate blocks (gram) of one split
    size_t lds;
    size_t off_mu, off_inv, off_sq, off_q, off_pkey, off_pidx, total;
};

static inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

static KnnPlan knn_plan(int N, int D, int k, int cus) {
    KnnPlan p;
    const int Np = plane_stride(N);
    p.direct = D <= KNN_DSMALL;
    p.kc = knn_kc(N, k);
    const int qb = p.direct ? KNN_T : KNN_QB, cb = p.direct ? KNN_T : KNN_CB;
    p.nqb = (N + qb - 1) / qb;
    const int ncb = (N + cb - 1) / cb;
    // two workgroups per CU where the query blocks alone give fewer than one
    int want = p.nqb >= cus ? 1 : (2 * cus + p.nqb - 1) / p.nqb;
    want = min(min(want, KNN_MAXSPLIT), ncb);
    const int per_blocks = (ncb + want - 1) / want;
    p.nsplit = (ncb + per_blocks - 1) / per_blocks;
    p.per = p.direct ? per_blocks * cb : per_blocks;
    p.P = p.direct ? p.nsplit : 2 * p.nsplit;
    p.lds = (size_t)2 * p.kc * KNN_T * 4 + (p.direct ? (size_t)KNN_DSMALL * KNN_T * 4 : 0);
    size_t o = 0;
    p.off_mu = o;   o += up256((size_t)Np * 8);
    p.off_inv = o;  o += up256((size_t)Np * 8);
    p.off_sq = o;   o += up256((size_t)Np * 4);
    p.off_q = o;    o += up256((size_t)D * Np * 4);
    p.off_pkey = o; o += up256((size_t)N * p.P * p.kc * 4);
    p.off_pidx = o; o += up256((size_t)N * p.P * p.kc * 4);
    p.total = o;
    return p;
}

static int knn_cus() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus <= 0)
        cus = 256;                       // sizes the split only (the workspace bound below never depends on it)
    return cus;
}

// the workspace does not depend on the device: sized for the most partial lists any split can give
static size_t knn_workspace_bound(int N, int D, int k) {
    const int Np = plane_stride(N);
    const size_t lists = (size_t)N * (2 * KNN_MAXSPLIT) * knn_kc(N, k) * 4;
    return 2 * up256((size_t)Np * 8) + up256((size_t)Np * 4) + up256((size_t)D * Np * 4) + 2 * up256(lists);
}

static int knn_check_shape(int N, int D, int k) {
    if (N < 2 || D < 1 || k < 1 || k >= N) return fail(CHEBGCN_EINVAL, "knn: bad shape (N = %d, D = %d, k = %d: 1 <= k < N)", N, D, k);
    if (k > KNN_KMAX) return fail(CHEBGCN_EUNSUPPORTED, "knn: k = %d, at most %d neighbours are served", k, KNN_KMAX);
    if ((int64_t)D * plane_stride(N) > 0x7fffffffLL || N > (1 << 24))
        return fail(CHEBGCN_EUNSUPPORTED, "knn: N = %d, D = %d beyond the served size", N, D);
    return CHEBGCN_OK;
}

}  // namespace chebgcn

using namespace chebgcn;

extern "C" size_t chebgcn_knn_workspace(int N, int D, int k) {
    if (N < 2 || D < 1 || k < 1 || k >= N || k > KNN_KMAX || (int64_t)D * plane_stride(N) > 0x7fffffffLL || N > (1 << 24)) return 0;
    return knn_workspace_bound(N, D, k);
}

extern "C" int chebgcn_knn(const float* feat, int N, int D, int k, int metric, float* dist_out, int32_t* idx_out, void* workspace,
                           size_t workspace_bytes, chebgcn_stream stream_) {
    const int rc = knn_check_shape(N, D, k);
    if (rc != CHEBGCN_OK) return rc;
    CG_REQUIRE(metric >= CHEBGCN_KNN_EUCLIDEAN && metric <= CHEBGCN_KNN_DOT, "knn: unknown metric %d", metric);
    CG_REQUIRE(feat && dist_out && idx_out && workspace, "knn: NULL argument");
    CG_REQUIRE(workspace_bytes >= knn_workspace_bound(N, D, k), "knn: workspace of %zu bytes, %zu needed", workspace_bytes,
               knn_workspace_bound(N, D, k));
    CG_REQUIRE((((uintptr_t)feat | (uintptr_t)workspace) & 15) == 0, "knn: feat and workspace must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    const int Np = plane_stride(N);
    const KnnPlan p = knn_plan(N, D, k, knn_cus());
    char* ws = (char*)workspace;
    double* mu = (double*)(ws + p.off_mu);
    double* inv = (double*)(ws + p.off_inv);
    float* sq = (float*)(ws + p.off_sq);
    float* Qn = (float*)(ws + p.off_q);
    float* pkey = (float*)(ws + p.off_pkey);
    int* pidx = (int*)(ws + p.off_pidx);
    const int euclid = metric == CHEBGCN_KNN_EUCLIDEAN;
    const bool copy = metric == CHEBGCN_KNN_COSINE || metric == CHEBGCN_KNN_CORRELATION;
    const float* Q = copy ? Qn : feat;

    note_dispatch("knn_prep_kernel");
    hipLaunchKernelGGL(knn_prep_kernel, dim3((Np + KNN_T - 1) / KNN_T), dim3(KNN_T), 0, stream, feat, N, Np, D, metric, mu, inv, sq,
                       Qn);
    CG_HIP(hipGetLastError());
    dim3 grid(p.nqb, p.nsplit);
    if (p.direct) {
        note_dispatch_more(p.nsplit > 1 ? "knn_direct_kernel<split>" : "knn_direct_kernel<whole>");
        CG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(knn_direct_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)p.lds));
        hipLaunchKernelGGL(knn_direct_kernel, grid, dim3(KNN_T), p.lds, stream, Q, N, Np, D, p.kc, p.per, euclid, p.P, pkey, pidx);
    } else {
        note_dispatch_more(p.nsplit > 1 ? "knn_gram_kernel<split>" : "knn_gram_kernel<whole>");
        CG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(knn_gram_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)p.lds));
        hipLaunchKernelGGL(knn_gram_kernel, grid, dim3(KNN_T), p.lds, stream, Q, sq, N, Np, D, p.kc, p.per, euclid, p.P, pkey, pidx);
    }
    CG_HIP(hipGetLastError());
    note_dispatch_more("knn_merge_refine_kernel");
    hipLaunchKernelGGL(knn_merge_refine_kernel, dim3((N + KNN_T / 64 - 1) / (KNN_T / 64)), dim3(KNN_T), 0, stream, feat, mu, inv, pkey,
                       pidx, N, Np, D, k, p.kc, p.P, metric, dist_out, idx_out);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_series_normalise(const float* series, int64_t Ttot, const int64_t* run_offsets, int R, int M, float scale,
                                        float* out, chebgcn_stream stream_) {
    CG_REQUIRE(series && run_offsets && out, "series_normalise: NULL argument");
    CG_REQUIRE(series != out, "series_normalise: in place");
    CG_REQUIRE(Ttot > 0 && R > 0 && R <= 65535 && M > 0 && Ttot * (int64_t)plane_stride(M) <= 0x7fffffffffLL,
               "series_normalise: bad shape (Ttot = %lld, R = %d, M = %d)", (long long)Ttot, R, M);
    const int Mp = plane_stride(M);
    note_dispatch("series_normalise_kernel");
    hipLaunchKernelGGL(series_normalise_kernel, dim3((Mp + KNN_T - 1) / KNN_T, R), dim3(KNN_T), 0, (hipStream_t)stream_, series,
                       (const long long*)run_offsets, M, Mp, scale, out);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}
