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
//            atomics, the result does not depend on the order of rows[] and is bit-identical from run to run.
#include "common.h"

namespace chebgcn {

constexpr int GW_T = 256;               // threads of the gather
constexpr int GW_U = 4;                 // 16-byte pieces per thread
constexpr int WS_T = 256;               // threads of the statistics kernels
constexpr int WS_CG = 8;                // channels a statistics workgroup accumulates (registers: 2 * 2 * WS_CG doubles)
constexpr int WS_ROWS = 512;            // series rows of one chunk (a chunk's partials are 2 * C * Mp doubles)

__device__ __forceinline__ long long clamp_row(long long r, long long last) { return r < 0 ? 0 : (r > last ? last : r); }

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
        if (e < CMq) {
            float4 r = v[u];
            if (Tables) {               // a rounded product, then a rounded sum: never one fma
                r.x = __fadd_rn(__fmul_rn(r.x, a[u].x), s[u].x);
                r.y = __fadd_rn(__fmul_rn(r.y, a[u].y), s[u].y);
                r.z = __fadd_rn(__fmul_rn(r.z, a[u].z), s[u].z);
                r.w = __fadd_rn(__fmul_rn(r.w, a[u].w), s[u].w);
            }
            const int m = 4 * (e % Mq);
            if (m + 3 >= M) {           // the pad of an output plane is zero whatever the operands hold there
                if (m >= M) r.x = 0.f;
                if (m + 1 >= M) r.y = 0.f;
                if (m + 2 >= M) r.z = 0.f;
                r.w = 0.f;
            }
            dst[e] = r;
        }
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
                for (int j = 1; j < N; ++j) {           // float32 adds in ascending j
                    r.x = __fadd_rn(r.x, v[j][u].x);
                    r.y = __fadd_rn(r.y, v[j][u].y);
                    r.z = __fadd_rn(r.z, v[j][u].z);
                    r.w = __fadd_rn(r.w, v[j][u].w);
                }
                if (N > 1) {                            // one correctly rounded division (n = 1: the plain gather's bits)
                    r.x = __fdiv_rn(r.x, (float)N);
                    r.y = __fdiv_rn(r.y, (float)N);
                    r.z = __fdiv_rn(r.z, (float)N);
                    r.w = __fdiv_rn(r.w, (float)N);
                }
                if (Tables) {                           // after the mean; a rounded product, then a rounded sum
                    r.x = __fadd_rn(__fmul_rn(r.x, a[u].x), s[u].x);
                    r.y = __fadd_rn(__fmul_rn(r.y, a[u].y), s[u].y);
                    r.z = __fadd_rn(__fmul_rn(r.z, a[u].z), s[u].z);
                    r.w = __fadd_rn(__fmul_rn(r.w, a[u].w), s[u].w);
                }
                const int m = 4 * (e % Mq);
                if (m + 3 >= M) {
                    if (m >= M) r.x = 0.f;
                    if (m + 1 >= M) r.y = 0.f;
                    if (m + 2 >= M) r.z = 0.f;
                    r.w = 0.f;
                }
                dst[e] = r;
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

// n[lead + row] += 1 per window (integer adds: the counts do not depend on the order of arrival).  lead = C - 1 + WS_CG zeros in
// front and 4 behind: n[lead + u - c] is in bounds for every row u < Ttot + 3 and every channel c < C + WS_CG - 1 the partial
// kernel's unrolled loads touch
__global__ void __launch_bounds__(256)
window_count_kernel(const long long* __restrict__ rows, long long S, long long last_row, int C, int* __restrict__ cnt) {
    const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
    if (w < S) atomicAdd(cnt + (C - 1 + WS_CG) + clamp_row(rows[w], last_row), 1);
}

// block (tile of 2 * WS_T vertices x group of WS_CG channels, chunk g of WS_ROWS rows): part[g][k][c][m], k = 0 the sum of
// n d, k = 1 the sum of n d^2 over the chunk's rows in ascending order
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
    double s1[WS_CG][2], s2[WS_CG][2];
#pragma unroll
    for (int j = 0; j < WS_CG; ++j) s1[j][0] = s1[j][1] = s2[j][0] = s2[j][1] = 0.0;
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
                const double q0 = d0 * d0, q1 = d1 * d1;
#pragma unroll
                for (int j = 0; j < WS_CG; ++j) {
                    if (j < nc) {
                        const int w = n[i - j + WS_CG - 1];
                        if (w != 0) {
                            const double wd = (double)w;
                            s1[j][0] = fma(wd, d0, s1[j][0]);
                            s1[j][1] = fma(wd, d1, s1[j][1]);
                            s2[j][0] = fma(wd, q0, s2[j][0]);
                            s2[j][1] = fma(wd, q1, s2[j][1]);
                        }
                    }
                }
            }
        }
    }
    const size_t slab = (size_t)C * Mp;
    double* p = part + (size_t)g * 2 * slab;
#pragma unroll
    for (int j = 0; j < WS_CG; ++j) {
        if (j < nc) {
            const size_t o = (size_t)(c0 + j) * Mp + m;
            *reinterpret_cast<double2*>(p + o) = make_double2(s1[j][0], s1[j][1]);
            *reinterpret_cast<double2*>(p + slab + o) = make_double2(s2[j][0], s2[j][1]);
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
        double a = 0.0, q = 0.0;
        for (int g = 0; g < G; ++g) {
            a += part[(size_t)g * 2 * slab + e];
            q += part[(size_t)g * 2 * slab + slab + e];
        }
        const double n = (double)S, da = a / n;
        mu = (double)series[m] + da;
        va = q / n - da * da;
        if (!(va > 0.0)) va = 0.0;
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

}  // namespace chebgcn

using namespace chebgcn;

extern "C" int chebgcn_gather_windows(const float* series, int64_t Ttot, const int64_t* rows, const int32_t* sample,
                                      const float* scale, const float* shift, float* out, int B, int M, int C,
                                      chebgcn_stream stream_) {
    CG_REQUIRE(series && rows && out, "gather_windows: NULL argument");
    CG_REQUIRE((scale != nullptr) == (shift != nullptr), "gather_windows: scale and shift come together (both or neither)");
    CG_REQUIRE(B > 0 && B <= 65535 && M > 0 && C > 0 && (int64_t)C * plane_stride(M) / 4 <= 0x7fffffffLL / 2,
               "gather_windows: bad shape (B = %d, M = %d, C = %d)", B, M, C);
    CG_REQUIRE(Ttot >= C, "gather_windows: a series of %lld time points holds no window of %d", (long long)Ttot, C);
    CG_REQUIRE((((uintptr_t)series | (uintptr_t)out | (uintptr_t)scale | (uintptr_t)shift) & 15) == 0,
               "gather_windows: series, tables and out must be 16-byte aligned");
    const int Mq = plane_stride(M) / 4, CMq = C * Mq;
    dim3 grid((CMq + GW_T * GW_U - 1) / (GW_T * GW_U), B);
    if (scale) {
        note_dispatch("gather_windows_kernel<tables>");
        hipLaunchKernelGGL(gather_windows_kernel<true>, grid, dim3(GW_T), 0, (hipStream_t)stream_, series,
                           (long long)(Ttot - C), (const long long*)rows, sample, scale, shift, out, M, Mq, CMq);
    } else {
        note_dispatch("gather_windows_kernel<plain>");
        hipLaunchKernelGGL(gather_windows_kernel<false>, grid, dim3(GW_T), 0, (hipStream_t)stream_, series,
                           (long long)(Ttot - C), (const long long*)rows, sample, scale, shift, out, M, Mq, CMq);
    }
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_gather_windows_mix(const float* series, int64_t Ttot, const int64_t* rows, const int32_t* cnt, int smax,
                                          const int32_t* sample, const float* scale, const float* shift, float* out, int B, int M,
                                          int C, chebgcn_stream stream_) {
    CG_REQUIRE(series && rows && out, "gather_windows_mix: NULL argument");
    CG_REQUIRE(cnt, "gather_windows_mix: NULL cnt (the number of sources of every window)");
    CG_REQUIRE(smax >= 1 && smax <= GWM_MAX, "gather_windows_mix: smax = %d, must be in [1, %d]", smax, GWM_MAX);
    CG_REQUIRE((scale != nullptr) == (shift != nullptr), "gather_windows_mix: scale and shift come together (both or neither)");
    CG_REQUIRE(B > 0 && B <= 65535 && M > 0 && C > 0 && (int64_t)C * plane_stride(M) / 4 <= 0x7fffffffLL / 2,
               "gather_windows_mix: bad shape (B = %d, M = %d, C = %d)", B, M, C);
    CG_REQUIRE(Ttot >= C, "gather_windows_mix: a series of %lld time points holds no window of %d", (long long)Ttot, C);
    CG_REQUIRE((((uintptr_t)series | (uintptr_t)out | (uintptr_t)scale | (uintptr_t)shift) & 15) == 0,
               "gather_windows_mix: series, tables and out must be 16-byte aligned");
    const int Mq = plane_stride(M) / 4, CMq = C * Mq;
    dim3 grid((CMq + GW_T * GW_U - 1) / (GW_T * GW_U), B);
    if (scale) {
        note_dispatch("gather_windows_mix_kernel<tables>");
        hipLaunchKernelGGL(gather_windows_mix_kernel<true>, grid, dim3(GW_T), 0, (hipStream_t)stream_, series,
                           (long long)(Ttot - C), (const long long*)rows, cnt, smax, sample, scale, shift, out, M, Mq, CMq);
    } else {
        note_dispatch("gather_windows_mix_kernel<plain>");
        hipLaunchKernelGGL(gather_windows_mix_kernel<false>, grid, dim3(GW_T), 0, (hipStream_t)stream_, series,
                           (long long)(Ttot - C), (const long long*)rows, cnt, smax, sample, scale, shift, out, M, Mq, CMq);
    }
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" size_t chebgcn_window_stats_workspace(int64_t Ttot, int M, int C) {
    if (Ttot <= 0 || M <= 0 || C <= 0 || Ttot > 0x7fffffffLL) return 0;
    return ws_count_bytes(Ttot, C) + (size_t)ws_chunks(Ttot) * 2 * C * plane_stride(M) * sizeof(double);
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
    note_dispatch_more("window_stats_finish_kernel");
    const size_t slab = (size_t)C * Mp;
    hipLaunchKernelGGL(window_stats_finish_kernel, dim3((unsigned)((slab + WS_T - 1) / WS_T)), dim3(WS_T), 0, stream, series, part,
                       G, (long long)S, M, Mp, C, mean, var, scale, shift);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}
