// What the window gathers share (series.hip, augment.hip): their launch shape, the clamp of a row read from memory, what happens
// to a 16-byte piece of a window before it is stored, the argument checks and the launch under a dispatch name.
#pragma once
#include "common.h"

namespace chebgcn {

constexpr int GW_T = 256;               // threads of the gather
constexpr int GW_U = 4;                 // 16-byte pieces per thread

__device__ __forceinline__ long long clamp_row(long long r, long long last) { return r < 0 ? 0 : (r > last ? last : r); }

// the tables (a rounded product, then a rounded sum: never one fma), the zero pad (the pad of an output plane is zero whatever
// the operands hold there), the store
template <bool Tables>
__device__ __forceinline__ void finish_piece(float4 r, float4 a, float4 s, int q, int M, float4* __restrict__ dst) {
    if (Tables) {
        r.x = __fadd_rn(__fmul_rn(r.x, a.x), s.x);
        r.y = __fadd_rn(__fmul_rn(r.y, a.y), s.y);
        r.z = __fadd_rn(__fmul_rn(r.z, a.z), s.z);
        r.w = __fadd_rn(__fmul_rn(r.w, a.w), s.w);
    }
    const int m = 4 * q;
    if (m + 3 >= M) {
        if (m >= M) r.x = 0.f;
        if (m + 1 >= M) r.y = 0.f;
        if (m + 2 >= M) r.z = 0.f;
        r.w = 0.f;
    }
    *dst = r;
}

// the checks the gather entries share (name: the entry's, as its messages spell it), and their grid
static int gather_args(const char* name, const void* series, const void* table, const void* out, const float* scale,
                       const float* shift, int B, int M, int C) {
    CG_REQUIRE(series && table && out, "%s: NULL argument", name);
    CG_REQUIRE((scale != nullptr) == (shift != nullptr), "%s: scale and shift come together (both or neither)", name);
    CG_REQUIRE(B > 0 && B <= 65535 && M > 0 && C > 0 && (int64_t)C * plane_stride(M) / 4 <= 0x7fffffffLL / 2,
               "%s: bad shape (B = %d, M = %d, C = %d)", name, B, M, C);
    CG_REQUIRE((((uintptr_t)series | (uintptr_t)out | (uintptr_t)scale | (uintptr_t)shift) & 15) == 0,
               "%s: series, tables and out must be 16-byte aligned", name);
    return CHEBGCN_OK;
}
static inline dim3 gather_grid(int CMq, int B) { return dim3((CMq + GW_T * GW_U - 1) / (GW_T * GW_U), B); }

// KERNEL<true> with tables, KERNEL<false> without, under its dispatch name; needs scale, grid and stream_ in scope
#define CG_LAUNCH_GATHER(KERNEL, ...)                                                                                 \
    do {                                                                                                              \
        if (scale) {                                                                                                  \
            note_dispatch(#KERNEL "<tables>");                                                                        \
            hipLaunchKernelGGL(KERNEL<true>, grid, dim3(GW_T), 0, (hipStream_t)stream_, __VA_ARGS__);                 \
        } else {                                                                                                      \
            note_dispatch(#KERNEL "<plain>");                                                                         \
            hipLaunchKernelGGL(KERNEL<false>, grid, dim3(GW_T), 0, (hipStream_t)stream_, __VA_ARGS__);                \
        }                                                                                                             \
        CG_HIP(hipGetLastError());                                                                                    \
    } while (0)

}  // namespace chebgcn
