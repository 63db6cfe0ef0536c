// The project's counter-based generator: one Philox4x32-10 block (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11).
// flocoder_amd/noise.py (philox4x32) is its host form.  Users and their counter regions:
//   ode.hip   the SDE samplers' normal field    counter (j, draw, sample id lo, sample id hi)
//   ode.hip   the likelihood's probe field      counter (j, probe, sample id lo, sample id hi), key = seed + FC_PROBE_KEY_OFFSET (mod 2^64)
//   ot_plan.hip   the plan sampler's uniforms   counter (k, draw, 0x4F54504C, 0xFFFFFFFF): a sample id with the top word all ones is negative
//   masks.hip   the inpainting masks            counter (j, region, sample id lo, sample id hi), key = seed + FC_MASK_KEY_OFFSET (mod 2^64);
//               region 0 the type and the stroke / rectangle counts, 1 the 'noise' pixels, 2 the rectangles, 3 + s brush stroke s
//               (j = 0, 1 its start, j = 2 + t its step t): the list is at the head of masks.hip
//   rvq_train.hip   the codebook draws          counter (0 | 1, draw index, level, N), key = seed + FC_CODEBOOK_KEY_OFFSET (mod 2^64): the
//               four multipliers / addends of the bijection that is cycle-walked into [0, N) (codebook_draw)
// The augmentation draws (key = seed + FC_AUG_KEY_OFFSET, counter (j, region, sample id)) are made on the host alone (noise.py): augment.hip
// reads their integer table and includes nothing of this file.
#pragma once
#include <hip/hip_runtime.h>

namespace fc {

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

}  // namespace fc
