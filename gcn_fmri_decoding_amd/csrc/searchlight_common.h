// What every searchlight kernel shares (searchlight.hip, searchlight_lda.hip, searchlight_rdm.hip, searchlight_svm.hip and
// searchlight_ball.h): the limits of one call, the clamp that keeps a pointer read from memory inside its array, and the hit tally.
#pragma once
#include <limits.h>

#include "common.h"

namespace chebgcn {

constexpr int SL_CMAX = 32;                 // classes
constexpr int SL_NMAX = 65535;              // models (cells) of one call: a grid dimension
constexpr int SL_TILES = 65535;             // 64-sample tiles of a model's test samples (grid.y of searchlight_score_kernel)
constexpr int SL_GMAX = 1 << 20;            // groups

__device__ __forceinline__ int sl_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

// The hit tally, called by every lane of a wave: key = group * C + label where the lane's test sample is live, was given its label
// and its group lies in [0, G), -1 otherwise.  correct[group][label][u] += 1 per hit -- one int32 atomic per distinct key of the
// wave (ballot, readlane of the first hit's key, the lanes that share it counted at once).
__device__ __forceinline__ void sl_tally(int32_t* correct, int key, int U, int u, int lane) {
    unsigned long long left = __ballot(key >= 0);
    while (left) {
        const int leader = __builtin_ctzll(left);
        const int kk = __builtin_amdgcn_readlane(key, leader);
        const unsigned long long same = __ballot(key == kk);
        if (lane == leader) atomicAdd(correct + (size_t)kk * U + u, (int)__popcll(same));
        left &= ~same;
    }
}

}  // namespace chebgcn
