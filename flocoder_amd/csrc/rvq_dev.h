// The one nearest-codeword search of the residual quantiser: rvq.hip (fc_rvq_quantize) and rvq_train.hip (codebook fitting) both call it,
// so a training step's assignments are fc_rvq_quantize's in every bit.
#pragma once
#include <hip/hip_runtime.h>

namespace fc {

constexpr int RVQ_MAXD = 16;

// index of the codeword of cl [K][D] nearest to r in squared Euclidean distance (fp32, summed in index order), first index on ties
__device__ __forceinline__ int rvq_nearest(const float (&r)[RVQ_MAXD], const float* cl, int K, int D) {
    float best = INFINITY;
    int bi = 0;
    for (int k = 0; k < K; ++k) {
        float dist = 0.f;
#pragma unroll
        for (int d = 0; d < RVQ_MAXD; ++d)
            if (d < D) { const float t = r[d] - cl[k * D + d]; dist += t * t; }
        if (dist < best) { best = dist; bi = k; }
    }
    return bi;
}

}  // namespace fc
