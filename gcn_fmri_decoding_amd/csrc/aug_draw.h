// The counter-based generator of include/chebgcn.h (chebgcn_aug_draw), one definition for every kernel that draws from it:
// the augmented windows of augment.hip and the Monte-Carlo dropout masks of head.hip.  series.aug_draw is its NumPy restatement.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/chebgcn.h"

namespace chebgcn {

__device__ __forceinline__ uint32_t aug_fin(uint32_t x) {
    x ^= x >> 16;
    x *= CHEBGCN_AUG_MUL1;
    x ^= x >> 15;
    x *= CHEBGCN_AUG_MUL2;
    x ^= x >> 16;
    return x;
}

// the two key words of window i at (seed, refill): everything of a draw that does not depend on its index d
struct AugKeys {
    uint32_t k0, k1;
};

__device__ __forceinline__ AugKeys aug_keys(uint32_t seed, uint32_t refill, uint32_t i) {
    const uint32_t a = aug_fin(aug_fin(seed) + refill);
    AugKeys k;
    k.k0 = aug_fin(a + i);
    k.k1 = aug_fin((a ^ CHEBGCN_AUG_KEY) + i * CHEBGCN_AUG_WINDOW);
    return k;
}

__device__ __forceinline__ uint32_t aug_draw(AugKeys k, uint32_t d) { return aug_fin(aug_fin(k.k0 + d) ^ k.k1); }

}  // namespace chebgcn
