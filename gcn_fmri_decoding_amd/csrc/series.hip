// Training on scans (models_gcn.base_model.stage_windows / fit_series): the two kernels behind a dataset that IS windows of scans.
//
// series is every run of a dataset concatenated, [Ttot][Mp] planes in the model's internal vertex order (zero pad), and window w
// is the C consecutive planes from rows[w] on: x[w][c][m] = series[rows[w] + c][m] -- a window is ONE contiguous piece of
// C * Mp floats, never stored per window.
//
//   gather:  out[b][c][m] = x[rows[sample[b]]][c][m]  (* scale[c][m] + shift[c][m], two roundings), [B][C][Mp], pad zero:
//            a contiguous copy of C * Mp floats per window, 16 bytes per lane.
//   mix:     out[b][c][m] = (sum_{j < cnt[w]} series[rows[w][j] + c][m]) / cnt[w],  w = sample[b]: a window that is the mean of
//            up to 16 source windows (class balancing: a re-drawn copy at cnt = 1, a synthetic window above), float32 adds in
//            ascending j, one rounded division, then the tables: cnt + 1 windows of HBM traffic per output window.
//   stats:   mean / population variance over the S windows for every (c, m), without building a window: with n[t] = how many
//            windows start at row t,  sum_w f(x[w][c][m]) = sum_u n[u - c] f(series[u][m]):  ONE pass over the series, every
//            plane read once per group of 8 channels however much the windows overlap.  Sums run in float64 on the deviations
//            d = series[u][m] - series[0][m] (a vertex that is constant over time has d = 0 and variance exactly 0; no
//            cancellation against a large mean), in ascending u inside a chunk of rows, chunks added in index order: no float
//            atomics, the result does not depend on the order of rows[] and is bit-identical from run to run.  Every sum is
//            carried as an unevaluated pair (hi, lo) of doubles (dd_add below): the variance is the small difference of
//            sum d^2 / S and (sum d / S)^2, and one rounding of either at ITS magnitude is an error of 2^-53 d^2 in the
//            variance -- more than the variance itself where the windows lie closer to each other than to series[0] (few
//            windows, folded windows, one window: variance 0).  The pairs keep the order of the sums and lose nothing to it.
#include "gather_piece.h"

namespace chebgcn {

constexpr int WS_T = 256;               // threads of the statistics kernels
constexpr int WS_CG = 8;                // channels a statistics workgroup accumulates (registers: 2 * 2 * 2 * WS_CG doubles)
constexpr int WS_ROWS = 512;            // series rows of one chunk (a chunk's partials are WS_PART * C * Mp doubles)
constexpr int WS_PART = 4;              // slabs of a chunk's partials: the heads of sum n d and sum n d^2, then their tails

// ---- what the gathers do to a piece (16 bytes of a window): float32 adds and divisions of one rounding each, then the epilogue
// (finish_piece, gather_piece.h) ---
__device__ __forceinline__ float4 add4(float4 a, float4 b) {
    return make_float4(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w));
}
__device__ __forceinline__ float4 div4(float4 a, float d) {
    return make_float4(__fdiv_rn(a.x, d), __fdiv_rn(a.y, d), __fdiv_rn(a.z, d), __fdiv_rn(a.w, d));
}

// ---- the statistics' sums: (h, l) += (th, tl), the heads by Knuth's branch-free TwoSum (its rounding error is exact), the error
// and the tails into l.  Explicitly rounded operations: nothing here may be re-associated or contracted.
__device__ __forceinline__ void dd_add(double& h, double& l, double th, double tl) {
    const double s = __dadd_rn(h, th);
    const double b = __dsub_rn(s, h);
    const double e = __dadd_rn(__dsub_rn(h, __dsub_rn(s, b)), __dsub_rn(th, b));
    h = s;
    l = __dadd_rn(l, __dadd_rn(e, tl));
}
// (h, l) with the same value and |l| at most half a unit in the last place of h
__device__ __forceinline__ void dd_norm(double& h, double& l) {
    const double s = __dadd_rn(h, l);
    const double b = __dsub_rn(s, h);
    l = __dadd_rn(__dsub_rn(h, __dsub_rn(s, b)), __dsub_rn(l, b));
    h = s;
}
// a * b as a pair: the rounded product and its exact error
__device__ __forceinline__ void dd_mul(double a, double b, double& h, double& l) {
    h = __dmul_rn(a, b);
    l = fma(a, b, -h);
}
// (h, l) / n as a pair, n an integer held exactly
__device__ __forceinline__ void dd_div(double h, double l, double n, double& qh, double& ql) {
    qh = __ddiv_rn(h, n);
    ql = __ddiv_rn(__dadd_rn(fma(-qh, n, h), l), n);
}

// block (piece of the window's C * Mp/4 float4s, window b)
template <bool Tables>
__global__ void __launch_bounds__(GW_T)
gather_windows_kernel(const float* __restrict__ series, long long last_row, const long long* __restrict__ rows,
                      const int32_t* __restrict__ sample, const float* __restrict__ scale, const float* __restrict__ shift,
                      float* __restrict__ out, int M, int Mq, int CMq) {
    const int b = blockIdx.y;
    const long long row = clamp_row(rows[sample ? sample[b] : b], last_row);
    const float4* src = reinterpret_cast<const float4*>(series) + row * Mq;         // Mp is a multiple of 32 floats: 16-byte aligned
    float4* dst = reinterpret_cast<float4*>(out) + (long long)b * CMq;
    const int e0 = blockIdx.x * (GW_T * GW_U) + threadIdx.x;
    float4 v[GW_U], a[GW_U], s[GW_U];
#pragma unroll
    for (int u = 0; u < GW_U; ++u) {
        const int e = e0 + u * GW_T;
        if (e < CMq) {
            v[u] = src[e];
            if (Tables) {
                a[u] = reinterpret_cast<const float4*>(scale)[e];
                s[u] = reinterpret_cast<const float4*>(shift)[e];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < GW_U; ++u) {
        const int e = e0 + u * GW_T;
        if (e < CMq) finish_piece<Tables>(v[u], a[u], s[u], e % Mq, M, dst + e);
    }
}

// ---- the mix gather: an output window is the mean of n <= GWM_MAX source windows (series.balance_plan) ------------------------
// One window's n is the same for every thread of its blocks, so the kernel branches ONCE on it into a body whose source count
// is a compile-time constant: the n loads of a piece are straight-line code, all issued before the first add (a per-load
// "j < n" test would make the compiler wait for every load on its own).  Pieces in flight per thread: n * U float4s <= 16.
constexpr int GWM_MAX = 16;

template <bool Tables, int N>
__device__ __forceinline__ void mix_pieces(const float4* __restrict__ series4, long long last_row,
                                           const long long* __restrict__ rw, const float* __restrict__ scale,
                                           const float* __restrict__ shift, float4* __restrict__ dst, int M, int Mq, int CMq) {
    constexpr int U = N <= 4 ? GW_U : (N <= 8 ? GW_U / 2 : GW_U / 4);
    const float4* src[N];
#pragma unroll
    for (int j = 0; j < N; ++j) src[j] = series4 + clamp_row(rw[j], last_row) * Mq;
    for (int p = 0; p < GW_U / U; ++p) {
        const int e0 = blockIdx.x * (GW_T * GW_U) + p * (GW_T * U) + threadIdx.x;
        float4 v[N][U], a[U], s[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * GW_T;
            if (e < CMq) {
#pragma unroll
                for (int j = 0; j < N; ++j) v[j][u] = src[j][e];
                if (Tables) {
                    a[u] = reinterpret_cast<const float4*>(scale)[e];
                    s[u] = reinterpret_cast<const float4*>(shift)[e];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * GW_T;
            if (e < CMq) {
                float4 r = v[0][u];
#pragma unroll
                for (int j = 1; j < N; ++j) r = add4(r, v[j][u]);           // float32 adds in ascending j
                if (N > 1) r = div4(r, (float)N);       // one correctly rounded division (n = 1: the plain gather's bits)
                finish_piece<Tables>(r, a[u], s[u], e % Mq, M, dst + e);    // the tables come after the mean
            }
        }
    }
}

// block (piece of the window's C * Mp/4 float4s, window b); rows [.][smax], cnt [.]: a count outside [1, smax] is clamped into it
template <bool Tables>
__global__ void __launch_bounds__(GW_T)
gather_windows_mix_kernel(const float* __restrict__ series, long long last_row, const long long* __restrict__ rows,
                          const int32_t* __restrict__ cnt, int smax, const int32_t* __restrict__ sample,
                          const float* __restrict__ scale, const float* __restrict__ shift, float* __restrict__ out, int M, int Mq,
                          int CMq) {
    const int b = blockIdx.y;
    const long long w = sample ? sample[b] : b;
    int n = cnt[w];
    n = n < 1 ? 1 : (n > smax ? smax : n);
    const long long* rw = rows + w * smax;
    const float4* series4 = reinterpret_cast<const float4*>(series);
    float4* dst = reinterpret_cast<float4*>(out) + (long long)b * CMq;
#define CG_MIX_CASE(N) case N: mix_pieces<Tables, N>(series4, last_row, rw, scale, shift, dst, M, Mq, CMq); break;
    switch (n) {
        CG_MIX_CASE(1) CG_MIX_CASE(2) CG_MIX_CASE(3) CG_MIX_CASE(4) CG_MIX_CASE(5) CG_MIX_CASE(6) CG_MIX_CASE(7) CG_MIX_CASE(8)
        CG_MIX_CASE(9) CG_MIX_CASE(10) CG_MIX_CASE(11) CG_MIX_CASE(12) CG_MIX_CASE(13) CG_MIX_CASE(14) CG_MIX_CASE(15)
        CG_MIX_CASE(16)
    }
#undef CG_MIX_CASE
    static_assert(GWM_MAX == 16, "one case per source count");
}

// ---- the indexed gather: a window is a LIST of rows (events.match_events) ------------------------------------------------------
// idx [S][Cin], Cin = C * fold: channel c of window s is the mean of the fold rows idx[s][f * C + c] (a trial padded by
// repeating its last volume, a chunk that straddles a rest period, TRstep sub-windows), and an output window the mean of n such
// windows (src [.][smax], cnt [.]: series.balance_plan's indices into idx; src == NULL: window w is its own single source).  A
// plane is still Mp contiguous floats, so the loads stay 16 bytes per lane and coalesced: only the row of a (window, channel)
// comes from the table -- one 8-byte load that a whole plane's lanes share.  Like the mix gather the kernel branches ONCE per
// workgroup on (fold, n) into a body whose counts are compile-time constants and whose fold * n loads of a piece are all
// issued before the first add; counts without a body of their own take the generic loop.  Every window index is clamped into
// [0, S - 1] and every row into [0, Ttot - 1]: nothing read from memory is an address or a trip count unchecked.
constexpr int GWI_MAX = 16;             // fold and n at most

struct IndexedArgs {
    const float4* series4;
    long long last_row;                 // Ttot - 1
    const long long* idx;               // [S][Cin]
    long long last_win;                 // S - 1
    int Cin, C, M, Mq, CMq;
};

// sw[j]: the (clamped) source windows of this workgroup's output window
template <bool Tables, int FOLD, int N>
__device__ __forceinline__ void indexed_pieces(const IndexedArgs& A, const long long* sw, const float* __restrict__ scale,
                                               const float* __restrict__ shift, float4* __restrict__ dst) {
    constexpr int L = FOLD * N;
    constexpr int U = L <= 4 ? GW_U : (L <= 8 ? GW_U / 2 : GW_U / 4);
    const long long* ir[N];
#pragma unroll
    for (int j = 0; j < N; ++j) ir[j] = A.idx + sw[j] * A.Cin;
    for (int p = 0; p < GW_U / U; ++p) {
        const int e0 = blockIdx.x * (GW_T * GW_U) + p * (GW_T * U) + threadIdx.x;
        float4 v[N][FOLD][U], a[U], s[U];
        int q[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * GW_T;
            if (e < A.CMq) {
                const int c = e / A.Mq;
                q[u] = e - c * A.Mq;
#pragma unroll
                for (int j = 0; j < N; ++j)
#pragma unroll
                    for (int f = 0; f < FOLD; ++f)
                        v[j][f][u] = A.series4[clamp_row(ir[j][f * A.C + c], A.last_row) * A.Mq + q[u]];
                if (Tables) {
                    a[u] = reinterpret_cast<const float4*>(scale)[e];
                    s[u] = reinterpret_cast<const float4*>(shift)[e];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * GW_T;
            if (e < A.CMq) {
                float4 r;
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    float4 w = v[j][0][u];
#pragma unroll
                    for (int f = 1; f < FOLD; ++f) w = add4(w, v[j][f][u]);         // float32 adds in ascending f
                    if (FOLD > 1) w = div4(w, (float)FOLD);                        // one rounded division per level
                    r = j == 0 ? w : add4(r, w);                                   // ... in ascending j
                }
                if (N > 1) r = div4(r, (float)N);
                finish_piece<Tables>(r, a[u], s[u], q[u], A.M, dst + e);
            }
        }
    }
}

// any (fold, n) in [1, 16]^2, one piece at a time
template <bool Tables>
__device__ __forceinline__ void indexed_pieces_any(const IndexedArgs& A, int fold, int n, const long long* __restrict__ srcw,
                                                   long long w, const float* __restrict__ scale, const float* __restrict__ shift,
                                                   float4* __restrict__ dst) {
    for (int u = 0; u < GW_U; ++u) {
        const int e = blockIdx.x * (GW_T * GW_U) + u * GW_T + threadIdx.x;
        if (e >= A.CMq) continue;
        const int c = e / A.Mq, q = e - c * A.Mq;
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f), a = r, s = r;
        if (Tables) {
            a = reinterpret_cast<const float4*>(scale)[e];
            s = reinterpret_cast<const float4*>(shift)[e];
        }
        for (int j = 0; j < n; ++j) {
            const long long sj = srcw ? clamp_row(srcw[j], A.last_win) : w;
            const long long* ir = A.idx + sj * A.Cin + c;
            float4 x = A.series4[clamp_row(ir[0], A.last_row) * A.Mq + q];
            for (int f = 1; f < fold; ++f) x = add4(x, A.series4[clamp_row(ir[(long long)f * A.C], A.last_row) * A.Mq + q]);
            if (fold > 1) x = div4(x, (float)fold);
            r = j == 0 ? x : add4(r, x);
        }
        if (n > 1) r = div4(r, (float)n);
        finish_piece<Tables>(r, a, s, q, A.M, dst + e);
    }
}

// block (piece of the window's C * Mp/4 float4s, window b).  W: the windows sample[] may name (the rows of src / cnt; S without)
template <bool Tables>
__global__ void __launch_bounds__(GW_T)
gather_windows_indexed_kernel(IndexedArgs A, int fold, const long long* __restrict__ src, const int32_t* __restrict__ cnt,
                              long long last_w, int smax, const int32_t* __restrict__ sample, const float* __restrict__ scale,
                              const float* __restrict__ shift, float* __restrict__ out) {
    const int b = blockIdx.y;
    const long long w = clamp_row(sample ? (long long)sample[b] : (long long)b, last_w);
    int n = 1;
    if (src) {
        n = cnt[w];
        n = n < 1 ? 1 : (n > smax ? smax : n);
    }
    const long long* srcw = src ? src + w * smax : nullptr;
    float4* dst = reinterpret_cast<float4*>(out) + (long long)b * A.CMq;
    long long sw[8];
#define CG_IDX_CASE(FOLD, N)                                                                                 \
    case FOLD * 32 + N: {                                                                                    \
        _Pragma("unroll") for (int j = 0; j < N; ++j) sw[j] = srcw ? clamp_row(srcw[j], A.last_win) : w;     \
        indexed_pieces<Tables, FOLD, N>(A, sw, scale, shift, dst);                                           \
    } break;
    switch (fold * 32 + n) {
        CG_IDX_CASE(1, 1) CG_IDX_CASE(1, 2) CG_IDX_CASE(1, 3) CG_IDX_CASE(1, 4)
        CG_IDX_CASE(1, 5) CG_IDX_CASE(1, 6) CG_IDX_CASE(1, 7) CG_IDX_CASE(1, 8)
        CG_IDX_CASE(2, 1) CG_IDX_CASE(2, 2) CG_IDX_CASE(2, 3) CG_IDX_CASE(2, 4)
        CG_IDX_CASE(3, 1) CG_IDX_CASE(4, 1)
        default: indexed_pieces_any<Tables>(A, fold, n, srcw, w, scale, shift, dst);
    }
#undef CG_IDX_CASE
}

// ---- the statistics of indexed windows -----------------------------------------------------------------------------------------
// Windows that are lists of rows have no "count of the windows that start here": the values the scaler sees are the FOLDED ones
// the gather forms in float32, so the kernel forms them the same way, window by window.  block (tile of 2 * WS_T vertices x
// channel c, chunk g of `chunk` windows): part[g][k][c][m] as window_stats_partial_kernel writes it, windows in ascending
// order; window_stats_finish_kernel adds the chunks in index order.
constexpr int WSI_CHUNKS = 32;          // chunks at most (a chunk's partials are WS_PART * C * Mp doubles)
constexpr int WSI_MIN = 16;             // windows of a chunk at least

template <int FOLD>                     // 0: any fold
__global__ void __launch_bounds__(WS_T)
window_stats_indexed_partial_kernel(const float* __restrict__ series, long long last_row, const long long* __restrict__ idx,
                                    long long S, int Cin, int fold_, int C, int Mp, long long chunk, double* __restrict__ part) {
    const int c = blockIdx.x % C, tile = blockIdx.x / C;
    const int m = 2 * (tile * WS_T + threadIdx.x);
    const int g = blockIdx.y;
    if (m >= Mp) return;
    const int fold = FOLD ? FOLD : fold_;
    const long long w0 = (long long)g * chunk, w1 = min(w0 + chunk, S);
    const float2 base = *reinterpret_cast<const float2*>(series + m);
    const double k0 = (double)base.x, k1 = (double)base.y;
    double s1[2] = {0.0, 0.0}, s2[2] = {0.0, 0.0}, c1[2] = {0.0, 0.0}, c2[2] = {0.0, 0.0};
    for (long long wb = w0; wb < w1; wb += 4) {
        float2 x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long* ir = idx + min(wb + i, w1 - 1) * Cin + c;
            x[i] = *reinterpret_cast<const float2*>(series + clamp_row(ir[0], last_row) * Mp + m);
            if (FOLD == 2) {
                const float2 y = *reinterpret_cast<const float2*>(series + clamp_row(ir[C], last_row) * Mp + m);
                x[i].x = __fdiv_rn(__fadd_rn(x[i].x, y.x), 2.f);
                x[i].y = __fdiv_rn(__fadd_rn(x[i].y, y.y), 2.f);
            } else if (FOLD == 0) {
                for (int f = 1; f < fold; ++f) {
                    const float2 y = *reinterpret_cast<const float2*>(series + clamp_row(ir[(long long)f * C], last_row) * Mp + m);
                    x[i].x = __fadd_rn(x[i].x, y.x);
                    x[i].y = __fadd_rn(x[i].y, y.y);
                }
                if (fold > 1) {
                    x[i].x = __fdiv_rn(x[i].x, (float)fold);
                    x[i].y = __fdiv_rn(x[i].y, (float)fold);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (wb + i < w1) {
                const double d0 = (double)x[i].x - k0, d1 = (double)x[i].y - k1;
                double q0, r0, q1, r1;
                dd_mul(d0, d0, q0, r0);
                dd_mul(d1, d1, q1, r1);
                dd_add(s1[0], c1[0], d0, 0.0);
                dd_add(s1[1], c1[1], d1, 0.0);
                dd_add(s2[0], c2[0], q0, r0);
                dd_add(s2[1], c2[1], q1, r1);
            }
        }
    }
    const size_t slab = (size_t)C * Mp, o = (size_t)c * Mp + m;
    double* p = part + (size_t)g * WS_PART * slab;
    *reinterpret_cast<double2*>(p + o) = make_double2(s1[0], s1[1]);
    *reinterpret_cast<double2*>(p + slab + o) = make_double2(s2[0], s2[1]);
    *reinterpret_cast<double2*>(p + 2 * slab + o) = make_double2(c1[0], c1[1]);
    *reinterpret_cast<double2*>(p + 3 * slab + o) = make_double2(c2[0], c2[1]);
}

static inline long long wsi_chunk(int64_t S) {
    const long long c = (S + WSI_CHUNKS - 1) / WSI_CHUNKS;
    return c < WSI_MIN ? WSI_MIN : c;
}
static inline int wsi_chunks(int64_t S) { return (int)((S + wsi_chunk(S) - 1) / wsi_chunk(S)); }

// n[lead + row] += 1 per window (integer adds: the counts do not depend on the order of arrival).  lead = C - 1 + WS_CG zeros in
// front and 4 behind: n[lead + u - c] is in bounds for every row u < Ttot + 3 and every channel c < C + WS_CG - 1 the partial
// kernel's unrolled loads touch
__global__ void __launch_bounds__(256)
window_count_kernel(const long long* __restrict__ rows, long long S, long long last_row, int C, int* __restrict__ cnt) {
    const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
    if (w < S) atomicAdd(cnt + (C - 1 + WS_CG) + clamp_row(rows[w], last_row), 1);
}

// block (tile of 2 * WS_T vertices x group of WS_CG channels, chunk g of WS_ROWS rows): part[g][k][c][m], k = 0 the sum of
// n d, k = 1 the sum of n d^2 over the chunk's rows in ascending order (their heads; k = 2, 3: their tails)
__global__ void __launch_bounds__(WS_T)
window_stats_partial_kernel(const float* __restrict__ series, long long Ttot, const int* __restrict__ cnt, int C, int Mp,
                            int ncg, double* __restrict__ part) {
    const int tile = blockIdx.x / ncg, c0 = (blockIdx.x % ncg) * WS_CG;
    const int m = 2 * (tile * WS_T + threadIdx.x);
    const int g = blockIdx.y;
    const long long u0 = (long long)g * WS_ROWS, u1 = min(u0 + (long long)WS_ROWS, Ttot);
    if (m >= Mp) return;
    const float2 base = *reinterpret_cast<const float2*>(series + m);
    const double k0 = (double)base.x, k1 = (double)base.y;
    double s1[WS_CG][2], s2[WS_CG][2], c1[WS_CG][2], c2[WS_CG][2];
#pragma unroll
    for (int j = 0; j < WS_CG; ++j) s1[j][0] = s1[j][1] = s2[j][0] = s2[j][1] = c1[j][0] = c1[j][1] = c2[j][0] = c2[j][1] = 0.0;
    const int nc = min(WS_CG, C - c0);
    for (long long u = u0; u < u1; u += 4) {
        float2 x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = *reinterpret_cast<const float2*>(series + min(u + i, Ttot - 1) * Mp + m);
        // the counts these four rows need, one batch of loads (the same for every thread): row u + i is channel c0 + j of the
        // windows that start at u + i - c0 - j
        const int* nb = cnt + (C - 1 + WS_CG) + u - c0 - (WS_CG - 1);
        int n[WS_CG + 3];
#pragma unroll
        for (int k = 0; k < WS_CG + 3; ++k) n[k] = nb[k];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (u + i < u1) {
                const double d0 = (double)x[i].x - k0, d1 = (double)x[i].y - k1;
                double q0, r0, q1, r1;                                  // d^2 = q + r exactly
                dd_mul(d0, d0, q0, r0);
                dd_mul(d1, d1, q1, r1);
#pragma unroll
                for (int j = 0; j < WS_CG; ++j) {
                    if (j < nc) {
                        const int w = n[i - j + WS_CG - 1];
                        if (w != 0) {
                            const double wd = (double)w;
                            double ph, pl;
                            dd_mul(wd, d0, ph, pl);
                            dd_add(s1[j][0], c1[j][0], ph, pl);
                            dd_mul(wd, d1, ph, pl);
                            dd_add(s1[j][1], c1[j][1], ph, pl);
                            dd_mul(wd, q0, ph, pl);
                            dd_add(s2[j][0], c2[j][0], ph, fma(wd, r0, pl));
                            dd_mul(wd, q1, ph, pl);
                            dd_add(s2[j][1], c2[j][1], ph, fma(wd, r1, pl));
                        }
                    }
                }
            }
        }
    }
    const size_t slab = (size_t)C * Mp;
    double* p = part + (size_t)g * WS_PART * slab;
#pragma unroll
    for (int j = 0; j < WS_CG; ++j) {
        if (j < nc) {
            const size_t o = (size_t)(c0 + j) * Mp + m;
            *reinterpret_cast<double2*>(p + o) = make_double2(s1[j][0], s1[j][1]);
            *reinterpret_cast<double2*>(p + slab + o) = make_double2(s2[j][0], s2[j][1]);
            *reinterpret_cast<double2*>(p + 2 * slab + o) = make_double2(c1[j][0], c1[j][1]);
            *reinterpret_cast<double2*>(p + 3 * slab + o) = make_double2(c2[j][0], c2[j][1]);
        }
    }
}

// thread (c, m): the chunks' partials in index order, then the tables
__global__ void __launch_bounds__(WS_T)
window_stats_finish_kernel(const float* __restrict__ series, const double* __restrict__ part, int G, long long S, int M, int Mp,
                           int C, double* __restrict__ mean, double* __restrict__ var, float* __restrict__ scale,
                           float* __restrict__ shift) {
    const size_t slab = (size_t)C * Mp;
    const size_t e = (size_t)blockIdx.x * WS_T + threadIdx.x;
    if (e >= slab) return;
    const int m = (int)(e % Mp);
    double mu = 0.0, va = 0.0;
    float sc = 0.f, sh = 0.f;
    if (m < M) {
        double ah = 0.0, al = 0.0, qh = 0.0, ql = 0.0;
        for (int g = 0; g < G; ++g) {
            const double* p = part + (size_t)g * WS_PART * slab + e;
            dd_add(ah, al, p[0], p[2 * slab]);
            dd_add(qh, ql, p[slab], p[3 * slab]);
        }
        // mean deviation da = a / S and mean square q / S as pairs, da^2 as a pair; the variance is their difference, head
        // from head (exact where they nearly cancel) and tail from tail
        const double n = (double)S;
        dd_norm(ah, al);
        dd_norm(qh, ql);
        double dh, dl, mh, ml, wh, wl;
        dd_div(ah, al, n, dh, dl);
        dd_div(qh, ql, n, mh, ml);
        dd_mul(dh, dh, wh, wl);
        wl = fma(2.0 * dh, dl, wl);
        va = __dadd_rn(__dsub_rn(mh, wh), __dsub_rn(ml, wl));
        if (!(va > 0.0)) va = 0.0;
        double base = (double)series[m], me = 0.0;
        dd_add(base, me, dh, dl);       // series[0][m] + da, rounded once
        mu = __dadd_rn(base, me);
        if (va == 0.0) {                // sklearn's _handle_zeros_in_scale: a constant entry is shifted, not scaled
            sc = 1.f;
            sh = (float)(-mu);
        } else {
            const double sd = sqrt(va);
            sc = (float)(1.0 / sd);
            sh = (float)(-mu / sd);
        }
    }
    if (mean) mean[e] = mu;
    if (var) var[e] = va;
    scale[e] = sc;
    shift[e] = sh;
}

static inline size_t ws_count_bytes(int64_t Ttot, int C) {
    return (((size_t)Ttot + C - 1 + WS_CG + 4) * sizeof(int) + 15) & ~(size_t)15;
}
static inline int ws_chunks(int64_t Ttot) { return (int)((Ttot + WS_ROWS - 1) / WS_ROWS); }

// the last launch of both statistics entries: the chunks' partials into the four tables
static int stats_finish(const float* series, const double* part, int G, int64_t S, int M, int Mp, int C, double* mean,
                        double* var, float* scale, float* shift, hipStream_t stream) {
    note_dispatch_more("window_stats_finish_kernel");
    const size_t slab = (size_t)C * Mp;
    hipLaunchKernelGGL(window_stats_finish_kernel, dim3((unsigned)((slab + WS_T - 1) / WS_T)), dim3(WS_T), 0, stream, series, part,
                       G, (long long)S, M, Mp, C, mean, var, scale, shift);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

}  // namespace chebgcn

using namespace chebgcn;

extern "C" int chebgcn_gather_windows(const float* series, int64_t Ttot, const int64_t* rows, const int32_t* sample,
                                      const float* scale, const float* shift, float* out, int B, int M, int C,
                                      chebgcn_stream stream_) {
    if (int rc = gather_args("gather_windows", series, rows, out, scale, shift, B, M, C)) return rc;
    CG_REQUIRE(Ttot >= C, "gather_windows: a series of %lld time points holds no window of %d", (long long)Ttot, C);
    const int Mq = plane_stride(M) / 4, CMq = C * Mq;
    const dim3 grid = gather_grid(CMq, B);
    CG_LAUNCH_GATHER(gather_windows_kernel, series, (long long)(Ttot - C), (const long long*)rows, sample, scale, shift, out, M, Mq,
                     CMq);
    return CHEBGCN_OK;
}

extern "C" int chebgcn_gather_windows_mix(const float* series, int64_t Ttot, const int64_t* rows, const int32_t* cnt, int smax,
                                          const int32_t* sample, const float* scale, const float* shift, float* out, int B, int M,
                                          int C, chebgcn_stream stream_) {
    if (int rc = gather_args("gather_windows_mix", series, rows, out, scale, shift, B, M, C)) return rc;
    CG_REQUIRE(cnt, "gather_windows_mix: NULL cnt (the number of sources of every window)");
    CG_REQUIRE(smax >= 1 && smax <= GWM_MAX, "gather_windows_mix: smax = %d, must be in [1, %d]", smax, GWM_MAX);
    CG_REQUIRE(Ttot >= C, "gather_windows_mix: a series of %lld time points holds no window of %d", (long long)Ttot, C);
    const int Mq = plane_stride(M) / 4, CMq = C * Mq;
    const dim3 grid = gather_grid(CMq, B);
    CG_LAUNCH_GATHER(gather_windows_mix_kernel, series, (long long)(Ttot - C), (const long long*)rows, cnt, smax, sample, scale,
                     shift, out, M, Mq, CMq);
    return CHEBGCN_OK;
}

extern "C" size_t chebgcn_window_stats_workspace(int64_t Ttot, int M, int C) {
    if (Ttot <= 0 || M <= 0 || C <= 0 || Ttot > 0x7fffffffLL) return 0;
    return ws_count_bytes(Ttot, C) + (size_t)ws_chunks(Ttot) * WS_PART * C * plane_stride(M) * sizeof(double);
}

extern "C" int chebgcn_window_stats(const float* series, int64_t Ttot, const int64_t* rows, int64_t S, double* mean, double* var,
                                    float* scale, float* shift, int M, int C, void* workspace, size_t workspace_bytes,
                                    chebgcn_stream stream_) {
    CG_REQUIRE(series && rows && scale && shift && workspace, "window_stats: NULL argument");
    CG_REQUIRE(S > 0 && S <= 0x7fffffffLL && M > 0 && C > 0 && Ttot <= 0x7fffffffLL, "window_stats: bad shape");
    CG_REQUIRE(Ttot >= C, "window_stats: a series of %lld time points holds no window of %d", (long long)Ttot, C);
    CG_REQUIRE(workspace_bytes >= chebgcn_window_stats_workspace(Ttot, M, C), "window_stats: workspace of %zu bytes, %zu needed",
               workspace_bytes, chebgcn_window_stats_workspace(Ttot, M, C));
    CG_REQUIRE((((uintptr_t)series | (uintptr_t)workspace) & 15) == 0, "window_stats: series and workspace must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    const int Mp = plane_stride(M), G = ws_chunks(Ttot), ncg = (C + WS_CG - 1) / WS_CG;
    CG_REQUIRE(G <= 65535, "window_stats: series too long");
    int* cnt = (int*)workspace;
    double* part = (double*)((char*)workspace + ws_count_bytes(Ttot, C));
    CG_HIP(hipMemsetAsync(cnt, 0, ws_count_bytes(Ttot, C), stream));
    note_dispatch("window_count_kernel");
    hipLaunchKernelGGL(window_count_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, stream, (const long long*)rows,
                       (long long)S, (long long)(Ttot - C), C, cnt);
    CG_HIP(hipGetLastError());
    note_dispatch_more("window_stats_partial_kernel");
    const int tiles = (Mp / 2 + WS_T - 1) / WS_T;
    hipLaunchKernelGGL(window_stats_partial_kernel, dim3(tiles * ncg, G), dim3(WS_T), 0, stream, series, (long long)Ttot, cnt, C,
                       Mp, ncg, part);
    CG_HIP(hipGetLastError());
    return stats_finish(series, part, G, S, M, Mp, C, mean, var, scale, shift, stream);
}

extern "C" int chebgcn_gather_windows_indexed(const float* series, int64_t Ttot, const int64_t* idx, int64_t S, int Cin, int fold,
                                              const int64_t* src, const int32_t* cnt, int64_t W, int smax, const int32_t* sample,
                                              const float* scale, const float* shift, float* out, int B, int M, int C,
                                              chebgcn_stream stream_) {
    if (int rc = gather_args("gather_windows_indexed", series, idx, out, scale, shift, B, M, C)) return rc;
    CG_REQUIRE((src != nullptr) == (cnt != nullptr), "gather_windows_indexed: src and cnt come together (both or neither)");
    CG_REQUIRE(!src || (smax >= 1 && smax <= GWI_MAX && W >= 1), "gather_windows_indexed: smax = %d, must be in [1, %d], W = %lld",
               smax, GWI_MAX, (long long)W);
    CG_REQUIRE(fold >= 1 && fold <= GWI_MAX, "gather_windows_indexed: fold = %d, must be in [1, %d]", fold, GWI_MAX);
    CG_REQUIRE((int64_t)Cin == (int64_t)C * fold, "gather_windows_indexed: Cin = %d is not C * fold = %d * %d", Cin, C, fold);
    CG_REQUIRE(S >= 1 && Ttot >= 1, "gather_windows_indexed: S = %lld windows of a series of %lld time points", (long long)S,
               (long long)Ttot);
    IndexedArgs A;
    A.series4 = reinterpret_cast<const float4*>(series);
    A.last_row = (long long)Ttot - 1;
    A.idx = (const long long*)idx;
    A.last_win = (long long)S - 1;
    A.Cin = Cin;
    A.C = C;
    A.M = M;
    A.Mq = plane_stride(M) / 4;
    A.CMq = C * A.Mq;
    const long long last_w = (src ? (long long)W : (long long)S) - 1;
    const dim3 grid = gather_grid(A.CMq, B);
    CG_LAUNCH_GATHER(gather_windows_indexed_kernel, A, fold, (const long long*)src, cnt, last_w, smax, sample, scale, shift, out);
    return CHEBGCN_OK;
}

extern "C" size_t chebgcn_window_stats_indexed_workspace(int64_t S, int M, int C) {
    if (S <= 0 || M <= 0 || C <= 0 || S > 0x7fffffffLL) return 0;
    return (size_t)wsi_chunks(S) * WS_PART * C * plane_stride(M) * sizeof(double);
}

extern "C" int chebgcn_window_stats_indexed(const float* series, int64_t Ttot, const int64_t* idx, int64_t S, int Cin, int fold,
                                            double* mean, double* var, float* scale, float* shift, int M, int C, void* workspace,
                                            size_t workspace_bytes, chebgcn_stream stream_) {
    CG_REQUIRE(series && idx && scale && shift && workspace, "window_stats_indexed: NULL argument");
    CG_REQUIRE(S > 0 && S <= 0x7fffffffLL && M > 0 && C > 0 && Ttot >= 1, "window_stats_indexed: bad shape");
    CG_REQUIRE(fold >= 1 && fold <= GWI_MAX, "window_stats_indexed: fold = %d, must be in [1, %d]", fold, GWI_MAX);
    CG_REQUIRE((int64_t)Cin == (int64_t)C * fold, "window_stats_indexed: Cin = %d is not C * fold = %d * %d", Cin, C, fold);
    CG_REQUIRE(workspace_bytes >= chebgcn_window_stats_indexed_workspace(S, M, C),
               "window_stats_indexed: workspace of %zu bytes, %zu needed", workspace_bytes,
               chebgcn_window_stats_indexed_workspace(S, M, C));
    CG_REQUIRE((((uintptr_t)series | (uintptr_t)workspace) & 15) == 0,
               "window_stats_indexed: series and workspace must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    const int Mp = plane_stride(M), G = wsi_chunks(S);
    const int tiles = (Mp / 2 + WS_T - 1) / WS_T;
    CG_REQUIRE((int64_t)tiles * C <= 0x7fffffffLL, "window_stats_indexed: bad shape");
    double* part = (double*)workspace;
    const dim3 grid(tiles * C, G);
    note_dispatch("window_stats_indexed_partial_kernel");
#define CG_WSI(FOLD)                                                                                                         \
    hipLaunchKernelGGL(window_stats_indexed_partial_kernel<FOLD>, grid, dim3(WS_T), 0, stream, series, (long long)Ttot - 1,  \
                       (const long long*)idx, (long long)S, Cin, fold, C, Mp, wsi_chunk(S), part)
    if (fold == 1) CG_WSI(1);
    else if (fold == 2) CG_WSI(2);
    else CG_WSI(0);
#undef CG_WSI
    CG_HIP(hipGetLastError());
    return stats_finish(series, part, G, S, M, Mp, C, mean, var, scale, shift, stream);
}
