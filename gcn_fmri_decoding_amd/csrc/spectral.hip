// Spectral graph filters (filter = 'fourier' / 'spline', lib_new/models_gcn.py:512-556): the graph Fourier transform as a
// dense fp32 GEMM on the gfx950 matrix cores, the per-frequency filter mix and its two gradients, and the spline
// parametrisation of the filter weights.
//
//   transform:   out[r][j] = sum_m in[r][m] * U[m][j]      (analysis, U = the eigenvectors [vertex][frequency])
//                out[r][j] = sum_m in[r][m] * U[j][m]      (synthesis, transpose != 0)
//                over R = B*F planes; U is [Mp][Mp] with zero padding
//   mix fwd:     yh[b][o][m]  = sum_fin W[m][o][fin] * xh[b][fin][m]
//   mix bwd_x:   dxh[b][fin][m] = sum_o W[m][o][fin] * dyh[b][o][m]
//   mix bwd_w:   dW[m][o][fin]  = sum_b dyh[b][o][m] * xh[b][fin][m]
//   spline:      W[m][c]  = sum_k Bs[m][k] * Wk[k][c]      and   dWk[k][c] = sum_m Bs[m][k] * dW[m][c]
//
// Every sum runs in a fixed order (an fmaf chain over the reduction index, the matrix instruction's own k order, or a
// fixed tree over four waves): repeated runs are bit-identical.  The pad [M, Mp) of an input plane is never read as data;
// the pad of every output plane is written as 0 (a zero-padded basis maps nothing there).
#include "common.h"

namespace chebgcn {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// --------------------------------------------------------------------------------------
// transform: C[R x Mp] = A[R x Mp] * Bm[Mp x Mp] on v_mfma_f32_32x32x2_f32
// --------------------------------------------------------------------------------------
// A wave owns a 32-row x 64-column tile of C (two 32x32 accumulators).  Lane l = (i = l & 31, h = l >> 5) loads the
// float4 A[row i][kb + 4h .. kb + 4h + 3] of its row; matrix step s (0..3) then takes k = kb + 4h + s from lane half h for
// both operands (any map of k onto (step, half) is a valid order as long as A and B agree; this one makes A a 16-byte
// load).  The B operand of step s is Bm[k][j]:
//   TB = false (analysis, Bm = U):    U[k][j0 + i]         one dword per step, a half-wave reads 128 contiguous bytes
//   TB = true  (synthesis, Bm = U^T): U[j0 + i][kb + 4h..] one float4 per four steps, like A
// The basis (Mp^2 floats: 590 KB at Mp = 384) is re-read by every row tile and stays in L2.
constexpr int TR_ROWS = 32, TR_COLS = 64, TR_UNROLL = 4;     // 4 x 8 = 32 k per loop turn (Mp is a multiple of 32)

template <bool TB>
__global__ void __launch_bounds__(256)
spectral_transform_kernel(const float* __restrict__ in, const float* __restrict__ U, float* __restrict__ out,
                          int R, int M, int Mp, int ntc) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.x * 4 + wave;
    const int tr = tile / ntc, tc = tile - tr * ntc;
    const int r0 = tr * TR_ROWS, j0 = tc * TR_COLS;
    if (r0 >= R) return;
    const int i = lane & 31, h = lane >> 5;
    const bool two = j0 + 32 < Mp;                        // second 32-column block inside the plane (wave-uniform)
    const int row = min(r0 + i, R - 1);                   // rows past R load a valid row and are not stored
    const float* arow = in + (size_t)row * Mp + 4 * h;

    f32x16 acc0, acc1;
#pragma unroll
    for (int q = 0; q < 16; ++q) { acc0[q] = 0.f; acc1[q] = 0.f; }

    for (int k0 = 0; k0 < Mp; k0 += 8 * TR_UNROLL) {
        float4 a[TR_UNROLL];
#pragma unroll
        for (int u = 0; u < TR_UNROLL; ++u) {
            const int kb = k0 + 8 * u + 4 * h;
            float4 v = *reinterpret_cast<const float4*>(arow + k0 + 8 * u);
            // the input pad is scratch: masked, not multiplied by the basis' zero rows (0 * NaN)
            a[u] = make_float4(kb < M ? v.x : 0.f, kb + 1 < M ? v.y : 0.f, kb + 2 < M ? v.z : 0.f, kb + 3 < M ? v.w : 0.f);
        }
        if (TB) {
            float4 b0[TR_UNROLL], b1[TR_UNROLL];
#pragma unroll
            for (int u = 0; u < TR_UNROLL; ++u) {
                b0[u] = *reinterpret_cast<const float4*>(U + (size_t)(j0 + i) * Mp + k0 + 8 * u + 4 * h);
                b1[u] = two ? *reinterpret_cast<const float4*>(U + (size_t)(j0 + 32 + i) * Mp + k0 + 8 * u + 4 * h)
                            : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < TR_UNROLL; ++u) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].x, b0[u].x, acc0, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].y, b0[u].y, acc0, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].z, b0[u].z, acc0, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].w, b0[u].w, acc0, 0, 0, 0);
                if (two) {
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].x, b1[u].x, acc1, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].y, b1[u].y, acc1, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].z, b1[u].z, acc1, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].w, b1[u].w, acc1, 0, 0, 0);
                }
            }
        } else {
            float b0[TR_UNROLL][4], b1[TR_UNROLL][4];
#pragma unroll
            for (int u = 0; u < TR_UNROLL; ++u)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float* p = U + (size_t)(k0 + 8 * u + 4 * h + s) * Mp + j0 + i;
                    b0[u][s] = p[0];
                    b1[u][s] = two ? p[32] : 0.f;
                }
#pragma unroll
            for (int u = 0; u < TR_UNROLL; ++u) {
                const float av[4] = {a[u].x, a[u].y, a[u].z, a[u].w};
#pragma unroll
                for (int s = 0; s < 4; ++s) acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], b0[u][s], acc0, 0, 0, 0);
                if (two) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], b1[u][s], acc1, 0, 0, 0);
                }
            }
        }
    }

    // accumulator register q of lane (i, h) is C[r0 + (q & 3) + 8 (q >> 2) + 4h][j0 + i]
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int r = r0 + (q & 3) + 8 * (q >> 2) + 4 * h;
        if (r < R) {
            float* orow = out + (size_t)r * Mp + j0 + i;
            orow[0] = acc0[q];
            if (two) orow[32] = acc1[q];
        }
    }
}

// --------------------------------------------------------------------------------------
// the per-frequency mix and its input gradient
// --------------------------------------------------------------------------------------
// out[b][o][m] = sum_i A_m[o][i] * in[b][i][m] with A_m = W[m] ([Fout][Fin], TR = false) or W[m]^T (TR = true).
// A thread owns one frequency m of MIX_NB windows and MIX_OT outputs; the planes are read along m (coalesced), the small
// matrices W[m] from L1 / L2.
constexpr int MIX_NB = 4, MIX_OT = 8;

template <bool TR>
__global__ void __launch_bounds__(256)
spectral_mix_kernel(const float* __restrict__ in, const float* __restrict__ W, float* __restrict__ out,
                    int B, int M, int Mp, int Fin, int Fout) {
    const int m = blockIdx.x * 64 + (threadIdx.x & 63);
    const int b0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * MIX_NB;
    const int o0 = blockIdx.z * MIX_OT;
    const int Ni = TR ? Fout : Fin, No = TR ? Fin : Fout;
    if (m >= Mp || b0 >= B) return;
    const bool live = m < M;
    float acc[MIX_NB][MIX_OT];
#pragma unroll
    for (int n = 0; n < MIX_NB; ++n)
#pragma unroll
        for (int t = 0; t < MIX_OT; ++t) acc[n][t] = 0.f;
    if (live) {
        const float* Wm = W + (size_t)m * Fout * Fin;
        for (int ii = 0; ii < Ni; ++ii) {
            float xv[MIX_NB];
#pragma unroll
            for (int n = 0; n < MIX_NB; ++n)
                xv[n] = b0 + n < B ? in[((size_t)(b0 + n) * Ni + ii) * Mp + m] : 0.f;
#pragma unroll
            for (int t = 0; t < MIX_OT; ++t) {
                const int o = o0 + t;
                const float w = o < No ? Wm[TR ? (size_t)ii * Fin + o : (size_t)o * Fin + ii] : 0.f;
#pragma unroll
                for (int n = 0; n < MIX_NB; ++n) acc[n][t] = fmaf(w, xv[n], acc[n][t]);
            }
        }
    }
#pragma unroll
    for (int n = 0; n < MIX_NB; ++n)
#pragma unroll
        for (int t = 0; t < MIX_OT; ++t)
            if (b0 + n < B && o0 + t < No) out[((size_t)(b0 + n) * No + o0 + t) * Mp + m] = acc[n][t];
}

// --------------------------------------------------------------------------------------
// the weight gradient: dW[m][o][fin] = sum_b dyh[b][o][m] * xh[b][fin][m]
// --------------------------------------------------------------------------------------
// Workgroup = 64 frequencies x a WG_OT x WG_IT block of (o, fin); wave w sums windows [w*nb, (w+1)*nb) in ascending
// order, then the four partial sums are added in wave order through LDS (no atomics).
constexpr int WG_OT = 8, WG_IT = 4;

__global__ void __launch_bounds__(256)
spectral_mix_bwd_w_kernel(const float* __restrict__ dyh, const float* __restrict__ xh, float* __restrict__ dW,
                          int B, int M, int Mp, int Fin, int Fout) {
    __shared__ float part[4][WG_OT * WG_IT][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = blockIdx.x * 64 + lane;
    const int o0 = blockIdx.y * WG_OT, f0 = blockIdx.z * WG_IT;
    const int nb = (B + 3) / 4;
    const int bb = min(wave * nb, B), be = min(bb + nb, B);
    float acc[WG_OT][WG_IT];
#pragma unroll
    for (int t = 0; t < WG_OT; ++t)
#pragma unroll
        for (int u = 0; u < WG_IT; ++u) acc[t][u] = 0.f;
    if (m < M) {
        for (int b = bb; b < be; ++b) {
            float dv[WG_OT], xv[WG_IT];
#pragma unroll
            for (int t = 0; t < WG_OT; ++t) dv[t] = o0 + t < Fout ? dyh[((size_t)b * Fout + o0 + t) * Mp + m] : 0.f;
#pragma unroll
            for (int u = 0; u < WG_IT; ++u) xv[u] = f0 + u < Fin ? xh[((size_t)b * Fin + f0 + u) * Mp + m] : 0.f;
#pragma unroll
            for (int t = 0; t < WG_OT; ++t)
#pragma unroll
                for (int u = 0; u < WG_IT; ++u) acc[t][u] = fmaf(dv[t], xv[u], acc[t][u]);
        }
    }
#pragma unroll
    for (int t = 0; t < WG_OT; ++t)
#pragma unroll
        for (int u = 0; u < WG_IT; ++u) part[wave][t * WG_IT + u][lane] = acc[t][u];
    __syncthreads();
    // element e = (ml * WG_OT + t) * WG_IT + u: consecutive threads store consecutive fin of one (m, o)
    for (int e = threadIdx.x; e < 64 * WG_OT * WG_IT; e += 256) {
        const int u = e % WG_IT, t = (e / WG_IT) % WG_OT, ml = e / (WG_IT * WG_OT);
        const int mm = blockIdx.x * 64 + ml, o = o0 + t, f = f0 + u;
        if (mm < M && o < Fout && f < Fin) {
            const int c = t * WG_IT + u;
            dW[((size_t)mm * Fout + o) * Fin + f] = ((part[0][c][ml] + part[1][c][ml]) + part[2][c][ml]) + part[3][c][ml];
        }
    }
}

// --------------------------------------------------------------------------------------
// spline parametrisation: W = Bs * Wk  and  dWk = Bs^T * dW   (Bs [M][K], Wk [K][C], W [M][C])
// --------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
spectral_spline_expand_kernel(const float* __restrict__ Bs, const float* __restrict__ Wk, float* __restrict__ W,
                              int M, int K, int C) {
    const int c = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;
    if (c >= C) return;
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc = fmaf(Bs[(size_t)m * K + k], Wk[(size_t)k * C + c], acc);
    W[(size_t)m * C + c] = acc;
}

__global__ void __launch_bounds__(256)
spectral_spline_expand_bwd_kernel(const float* __restrict__ Bs, const float* __restrict__ dW, float* __restrict__ dWk,
                                  int M, int K, int C) {
    const int c = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (c >= C) return;
    float acc = 0.f;
    for (int m = 0; m < M; ++m) acc = fmaf(Bs[(size_t)m * K + k], dW[(size_t)m * C + c], acc);
    dWk[(size_t)k * C + c] = acc;
}

}  // namespace chebgcn

using namespace chebgcn;

extern "C" int chebgcn_spectral_transform(const float* in, const float* basis, float* out, int R, int M, int transpose,
                                          chebgcn_stream stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CG_REQUIRE(in && basis && out, "spectral_transform: NULL argument");
    CG_REQUIRE(in != out, "spectral_transform: in place");
    CG_REQUIRE(R > 0 && M > 0 && M <= 32768, "spectral_transform: bad shape R=%d M=%d", R, M);
    const int Mp = plane_stride(M);
    const int ntc = (Mp + TR_COLS - 1) / TR_COLS;
    const int64_t tiles = (int64_t)((R + TR_ROWS - 1) / TR_ROWS) * ntc;
    CG_REQUIRE((tiles + 3) / 4 < (1ll << 31), "spectral_transform: R too large");
    dim3 grid((unsigned)((tiles + 3) / 4));
    if (transpose) {
        note_dispatch("spectral_transform_kernel<true>");
        hipLaunchKernelGGL(spectral_transform_kernel<true>, grid, dim3(256), 0, stream, in, basis, out, R, M, Mp, ntc);
    } else {
        note_dispatch("spectral_transform_kernel<false>");
        hipLaunchKernelGGL(spectral_transform_kernel<false>, grid, dim3(256), 0, stream, in, basis, out, R, M, Mp, ntc);
    }
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

static int mix_launch(bool tr, const float* in, const float* W, float* out, int B, int M, int Fin, int Fout,
                      hipStream_t stream) {
    const int Mp = plane_stride(M);
    const int No = tr ? Fin : Fout;
    CG_REQUIRE((B + 4 * MIX_NB - 1) / (4 * MIX_NB) <= 65535 && (No + MIX_OT - 1) / MIX_OT <= 65535,
               "spectral_mix: B=%d or %d outputs too large", B, No);
    dim3 grid((Mp + 63) / 64, (B + 4 * MIX_NB - 1) / (4 * MIX_NB), (No + MIX_OT - 1) / MIX_OT);
    if (tr) {
        note_dispatch("spectral_mix_kernel<true>");
        hipLaunchKernelGGL(spectral_mix_kernel<true>, grid, dim3(256), 0, stream, in, W, out, B, M, Mp, Fin, Fout);
    } else {
        note_dispatch("spectral_mix_kernel<false>");
        hipLaunchKernelGGL(spectral_mix_kernel<false>, grid, dim3(256), 0, stream, in, W, out, B, M, Mp, Fin, Fout);
    }
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_spectral_mix_fwd(const float* xh, const float* W, float* yh, int B, int M, int Fin, int Fout,
                                        chebgcn_stream stream) {
    CG_REQUIRE(xh && W && yh && xh != yh, "spectral_mix_fwd: NULL argument (or in place)");
    CG_REQUIRE(B > 0 && M > 0 && M <= 32768 && Fin > 0 && Fout > 0, "spectral_mix_fwd: bad shape");
    return mix_launch(false, xh, W, yh, B, M, Fin, Fout, (hipStream_t)stream);
}

extern "C" int chebgcn_spectral_mix_bwd_x(const float* dyh, const float* W, float* dxh, int B, int M, int Fin, int Fout,
                                          chebgcn_stream stream) {
    CG_REQUIRE(dyh && W && dxh && dyh != dxh, "spectral_mix_bwd_x: NULL argument (or in place)");
    CG_REQUIRE(B > 0 && M > 0 && M <= 32768 && Fin > 0 && Fout > 0, "spectral_mix_bwd_x: bad shape");
    return mix_launch(true, dyh, W, dxh, B, M, Fin, Fout, (hipStream_t)stream);
}

extern "C" int chebgcn_spectral_mix_bwd_w(const float* dyh, const float* xh, float* dW, int B, int M, int Fin, int Fout,
                                          chebgcn_stream stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CG_REQUIRE(dyh && xh && dW, "spectral_mix_bwd_w: NULL argument");
    CG_REQUIRE(B > 0 && M > 0 && M <= 32768 && Fin > 0 && Fout > 0, "spectral_mix_bwd_w: bad shape");
    CG_REQUIRE((Fout + WG_OT - 1) / WG_OT <= 65535 && (Fin + WG_IT - 1) / WG_IT <= 65535, "spectral_mix_bwd_w: too many filters");
    dim3 grid((M + 63) / 64, (Fout + WG_OT - 1) / WG_OT, (Fin + WG_IT - 1) / WG_IT);
    note_dispatch("spectral_mix_bwd_w_kernel");
    hipLaunchKernelGGL(spectral_mix_bwd_w_kernel, grid, dim3(256), 0, stream, dyh, xh, dW, B, M, plane_stride(M), Fin, Fout);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_spectral_spline_expand(const float* Bs, const float* Wk, float* W, int M, int K, int C,
                                              chebgcn_stream stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CG_REQUIRE(Bs && Wk && W, "spectral_spline_expand: NULL argument");
    CG_REQUIRE(M > 0 && M <= 65535 && K > 0 && C > 0, "spectral_spline_expand: bad shape");
    note_dispatch("spectral_spline_expand_kernel");
    hipLaunchKernelGGL(spectral_spline_expand_kernel, dim3((C + 255) / 256, M), dim3(256), 0, stream, Bs, Wk, W, M, K, C);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}

extern "C" int chebgcn_spectral_spline_expand_bwd(const float* Bs, const float* dW, float* dWk, int M, int K, int C,
                                                  chebgcn_stream stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CG_REQUIRE(Bs && dW && dWk, "spectral_spline_expand_bwd: NULL argument");
    CG_REQUIRE(M > 0 && K > 0 && K <= 65535 && C > 0, "spectral_spline_expand_bwd: bad shape");
    note_dispatch("spectral_spline_expand_bwd_kernel");
    hipLaunchKernelGGL(spectral_spline_expand_bwd_kernel, dim3((C + 255) / 256, K), dim3(256), 0, stream, Bs, dW, dWk, M, K, C);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}
