// Monte-Carlo dropout (models_gcn.base_model.predict_mc): the reduction of the S sampled logits of every window to its
// uncertainty measures.  (The sampled head itself is fc_fwd_dropout_kernel, csrc/head.hip.)
//
// One wave per window, lane c owns class c (C <= 64).  The samples are visited in order; what crosses lanes -- the maximum, the
// sum of the exponentials, the entropy terms -- goes through a butterfly of fixed shape, so two runs add the same numbers in the
// same order.  The per-lane running sums over the samples (the probabilities, the entropies) are float64: S additions of values
// in [0, log C] lose nothing that the float32 results could show.  No atomics.
#include "common.h"

namespace chebgcn {

constexpr int MC_CMAX = 64;             // classes: one lane each
constexpr int MC_SMAX = 1024;           // samples of one call
constexpr int MC_WAVES = 4;             // windows per workgroup
constexpr int MC_U = 4;                 // samples whose loads are in flight

// (value, class): is a a better maximum than b -- torch.argmax's rule (chebgcn_saliency_seed): the first maximum, a NaN counting
// as the largest value
__device__ __forceinline__ bool mc_better(float av, int ai, float bv, int bi) {
    const bool an = av != av, bn = bv != bv;
    if (an != bn) return an;
    if (an || av == bv) return ai < bi;
    return av > bv;
}

__device__ __forceinline__ void mc_argmax(float& v, int& i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(i, off, 64);
        if (mc_better(ov, oi, v, i)) {
            v = ov;
            i = oi;
        }
    }
}

template <typename T>
__device__ __forceinline__ T mc_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ void __launch_bounds__(MC_WAVES * 64)
mc_reduce_kernel(const float* __restrict__ z, int S, int B, int C, float* __restrict__ mean_p, float* __restrict__ entropy,
                 float* __restrict__ expected, float* __restrict__ mi, int32_t* __restrict__ label, int32_t* __restrict__ votes,
                 float* __restrict__ agreement) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * MC_WAVES + (threadIdx.x >> 6);
    if (b >= B) return;                                     // (a whole wave: nothing below synchronises across waves)
    const bool mine = lane < C;
    const float* col = z + (size_t)b * C + (mine ? lane : 0);
    const size_t step = (size_t)B * C;
    double psum = 0.0, hsum = 0.0;
    int nvote = 0;
    for (int s0 = 0; s0 < S; s0 += MC_U) {
        float zs[MC_U];
#pragma unroll
        for (int u = 0; u < MC_U; ++u) zs[u] = col[(size_t)min(s0 + u, S - 1) * step];
#pragma unroll
        for (int u = 0; u < MC_U; ++u) {
            const bool live = s0 + u < S;                   // (no branch: the MC_U chains of butterflies below are independent and interleave)
            const float v = mine ? zs[u] : -__builtin_inff();
            float m = v;
            int arg = lane;                                 // (a lane without a class holds -inf and an index behind every class)
            mc_argmax(m, arg);
            nvote += live && arg == lane;
            const float d = v - m;                          // <= 0; finite for finite logits
            const float e = mine ? expf(d) : 0.f;
            const float sum = mc_sum(e);                    // >= 1: the maximum contributes exp(0)
            const float p = e / sum;
            psum += live ? (double)p : 0.0;
            // H(p) = log(sum) - sum_c p_c (z_c - m): no log of a probability, so a class that underflowed to p = 0 adds 0 * d = 0
            const float t = mc_sum(mine ? p * d : 0.f);
            hsum += live ? (double)(logf(sum) - t) : 0.0;
        }
    }
    const double mp = psum / (double)S;
    const float mpf = (float)mp;
    const double h = mc_sum(mine && mp != 0.0 ? -mp * log(mp) : 0.0);          // 0 log 0 = 0; a NaN stays a NaN
    const double he = hsum / (double)S;
    float best = mine ? mpf : -__builtin_inff();
    int lab = lane;
    mc_argmax(best, lab);
    const int nl = __shfl(nvote, lab, 64);
    if (mine) {
        mean_p[(size_t)b * C + lane] = mpf;
        votes[(size_t)b * C + lane] = nvote;
    }
    if (lane == 0) {
        entropy[b] = (float)h;
        expected[b] = (float)he;
        mi[b] = h - he < 0.0 ? 0.f : (float)(h - he);       // >= 0 in exact arithmetic (Jensen), the rounding of two sums aside; a NaN stays
        label[b] = lab;
        agreement[b] = (float)nl / (float)S;
    }
}

}  // namespace chebgcn

using namespace chebgcn;

extern "C" int chebgcn_mc_reduce_supported(int S, int C) { return S >= 1 && S <= MC_SMAX && C >= 1 && C <= MC_CMAX; }

extern "C" int chebgcn_mc_reduce(const float* logits, int S, int B, int C, float* mean_p, float* entropy, float* expected_entropy,
                                 float* mutual_information, int32_t* label, int32_t* votes, float* agreement,
                                 chebgcn_stream stream_) {
    CG_REQUIRE(S > 0 && B > 0 && C > 0, "mc_reduce: bad shape (S = %d, B = %d, C = %d)", S, B, C);
    if (!chebgcn_mc_reduce_supported(S, C)) return CHEBGCN_EUNSUPPORTED;
    CG_REQUIRE(logits && mean_p && entropy && expected_entropy && mutual_information && label && votes && agreement,
               "mc_reduce: NULL argument");
    note_dispatch("mc_reduce_kernel");
    hipLaunchKernelGGL(mc_reduce_kernel, dim3((B + MC_WAVES - 1) / MC_WAVES), dim3(MC_WAVES * 64), 0, (hipStream_t)stream_, logits,
                       S, B, C, mean_p, entropy, expected_entropy, mutual_information, label, votes, agreement);
    CG_HIP(hipGetLastError());
    return CHEBGCN_OK;
}
