// Augmented training windows (series.WindowSet.augment): the two kernels that perturb a window while, or right after, it is
// gathered -- none of the copies is ever stored.
//
//   drop:     x[b][c][pos[v]] = drop_value (* scale + shift, two roundings) for the D vertices v the counter-based generator
//             draws for window win[b] (chebgcn_aug_draw, include/chebgcn.h): a SCATTER of D * C floats per window, in place on
//             the gathered batch.  A mask pass would read and write the whole batch (8 * B * C * Mp bytes) to change a
//             drop_rate share of it; the scatter writes B * D * C * 4 bytes and reads nothing of x.
//   reflect:  gather_windows with the channel map rho(c + tshift[w]): the window shifted in time by r inside its symmetric
//             reflection, np.pad(x, C, 'symmetric')[r + C : r + 2 C].  Channel c of the output is plane rho(c + r) of the same
//             C contiguous planes, so the loads stay 16 bytes per lane and coalesced; r = 0 is gather_windows' loads exactly.
#include "aug_draw.h"
#include "gather_piece.h"

namespace chebgcn {

constexpr int WD_T = 256;               // threads of the scatter: one draw each

// thread (draw t of the B * D of the batch): window b = t / D, draw d = t % D.  Two draws of one window may name the same
// vertex, and two threads then store to the same addresses: they store the SAME value (it depends on the channel and the
// position alone), so the race is benign and the result does not depend on which store lands last.  No atomics.
template <bool Tables>
__global__ void __launch_bounds__(WD_T)
window_drop_kernel(float* __restrict__ x, const int32_t* __restrict__ win, long long total, int M, int Mp, int C, int D,
                   uint32_t seed, uint32_t refill, const int32_t* __restrict__ pos, const float* __restrict__ scale,
                   const float* __restrict__ shift, float drop_value) {
    const long long t = (long long)blockIdx.x * WD_T + threadIdx.x;
    if (t >= total) return;
    const long long b = t / D;
    const uint32_t d = (uint32_t)(t - b * D);
    const uint32_t i = (uint32_t)win[b];                    // (enters the hash only: never an address)
    const uint32_t u = aug_draw(aug_keys(seed, refill, i), d);          // (aug_draw.h; series.drop_vertices restates it in NumPy)
    int p = (int)__umulhi(u, (uint32_t)M);                  // (u * M) >> 32: in [0, M) by construction
    if (pos) {
        p = pos[p];
        p = p < 0 ? 0 : (p > M - 1 ? M - 1 : p);            // read from memory: clamped before it is an address
    }
    float* dst = x + (size_t)b * C * Mp + p;
    for (int c = 0; c < C; ++c) {
        float v = drop_value;
        if (Tables) v = __fadd_rn(__fmul_rn(v, scale[(size_t)c * Mp + p]), shift[(size_t)c * Mp + p]);
        dst[(size_t)c * Mp] = v;
    }
}

// block (piece of the window's C * Mp/4 float4s, window b): gather_windows_kernel with the source plane rho(c + r)
template <bool Tables>
__global__ void __launch_bounds__(GW_T)
gather_windows_reflect_kernel(const float* __restrict__ series, long long last_row, const long long* __restrict__ rows,
                              const int32_t* __restrict__ tshift, const int32_t* __restrict__ sample,
                              const float* __restrict__ scale, const float* __restrict__ shift, float* __restrict__ out, int M,
                              int Mq, int C, int CMq) {
    const int b = blockIdx.y;
    const long long w = sample ? sample[b] : b;
    const long long row = clamp_row(rows[w], last_row);
    int r = tshift ? tshift[w] : 0;
    r = r < 0 ? 0 : (r > C - 1 ? C - 1 : r);
    const float4* src = reinterpret_cast<const float4*>(series) + row * Mq;         // Mp is a multiple of 32 floats: 16-byte aligned
    float4* dst = reinterpret_cast<float4*>(out) + (long long)b * CMq;
    const int e0 = blockIdx.x * (GW_T * GW_U) + threadIdx.x;
    float4 v[GW_U], a[GW_U], s[GW_U];
    int q[GW_U];
#pragma unroll
    for (int u = 0; u < GW_U; ++u) {
        const int e = e0 + u * GW_T;
        if (e < CMq) {
            const int c = e / Mq;
            q[u] = e - c * Mq;
            int j = c + r;                                                          // <= 2 C - 2
            j = j < C ? j : 2 * C - 1 - j;                                          // rho: in [0, C - 1]
            v[u] = src[j * Mq + q[u]];
            if (Tables) {
                a[u] = reinterpret_cast<const float4*>(scale)[e];
                s[u] = reinterpret_cast<const float4*>(shift)[e];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < GW_U; ++u) {
        const int e = e0 + u * GW_T;
        if (e < CMq) finish_piece<Tables>(v[u], a[u], s[u], q[u], M, dst + e);
    }
}

}  // namespace chebgcn

using namespace chebgcn;

extern "C" int chebgcn_window_drop(float* x, const int32_t* win, int B, int M, int C, int D, uint32_t seed, uint32_t refill,
                                   const int32_t* pos, const float* scale, const float* shift, float drop_value,
                                   chebgcn_stream stream_) {
    CG_REQUIRE(B >= 0 && D >= 0 && M > 0 && C > 0 && (int64_t)C * plane_stride(M) <= 0x7fffffffLL,
               "window_drop: bad shape (B = %d, M = %d, C = %d, D = %d)", B, M, C, D);
    CG_REQUIRE((scale != nullptr) == (shift != nullptr), "window_drop: scale and shift come together (both or neither)");
    if (B == 0 || D == 0) {             // nothing is drawn: no launch
        note_dispatch("");
        return CHEBGCN_OK;
    }
    CG_REQUIRE(x && win, "window_drop: NULL argument");
    const long long total = (long long)B * D;
    const long long blocks = (total + WD_T - 1) / WD_T;
    CG_REQUIRE(blocks <= 0x7fffffffLL, "window_drop: B * D = %lld draws are more than one launch takes", total);
    const dim3 grid((unsigned)blocks);
    const int Mp = plane_stride(M);
    if (scale) {
        note_dispatch("window_drop_kernel<tables>");
        hipLaunchKernelGGL(window_drop_kernel<true>, grid, dim3(WD_T), 0, (hipStream_t)stream_, x, win, total, M, Mp, C, D, seed,
                           refill, pos, scale, shift, drop_value);
    } else {
        note_dispatch("window_drop_kernel<plain>");
        hipLaunchKernelGGL(window_drop_kernel<false>, grid, dim3(WD_T), 0, (hipStream_t)stream_, x, win, total, M, Mp, C, D, seed,
                           refill, pos, scale, shift, drop_value);
    }
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_gather_windows_reflect(const float* series, int64_t Ttot, const int64_t* rows, const int32_t* tshift,
                                              const int32_t* sample, const float* scale, const float* shift, float* out, int B,
                                              int M, int C, chebgcn_stream stream_) {
    if (int rc = gather_args("gather_windows_reflect", series, rows, out, scale, shift, B, M, C)) return rc;
    CG_REQUIRE(Ttot >= C, "gather_windows_reflect: a series of %lld time points holds no window of %d", (long long)Ttot, C);
    const int Mq = plane_stride(M) / 4, CMq = C * Mq;
    const dim3 grid = gather_grid(CMq, B);
    CG_LAUNCH_GATHER(gather_windows_reflect_kernel, series, (long long)(Ttot - C), (const long long*)rows, tshift, sample, scale,
                     shift, out, M, Mq, C, CMq);
    return CHEBGCN_OK;
}
