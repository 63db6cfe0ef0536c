// Mini-batch OT pairing.
// Greedy (ot.py:63-78 compute_ot_pairing_approximate):
//   d = cdist(source, target) (L2);  for i = 0..B-1:  perm[i] = argmin over still-unused j of d[i][j] (first minimum).
// Kernel 1 forms the BxB distance matrix with direct differences (no |x|^2+|y|^2-2xy cancellation).
// Kernel 2 is the inherently sequential sweep: ONE wave64, column j owned by lane j%64, the `used` set as one
// bit per owned column in a register, (value, index) lexicographic min by cross-lane shuffles -- no LDS,
// no barriers, next row prefetched while the current one is reduced.
//
// Plans: ot_plan.hip (entropic plans, sampling from a plan) uses the squared-distance kernels and the sweep with the comparison turned round.
//
// Exact: c = squared distances (the same kernels with SQ set, non-finite entries stored as FLT_MAX), then the linear assignment
// solver `ot_assign_kernel` below: shortest augmenting paths with fp64 duals, one wave64, every loop bounded by B.
#include <float.h>

#include "common.h"

namespace fc {

constexpr int OT_T = 16, OT_K = 64;

// grid (ceil(B/16), ceil(B/16)), 256 threads: thread (r, c) of a 16x16 tile.  SQ: squared distances for the exact pairing.
template <bool SQ = false>
__global__ void __launch_bounds__(256) ot_dist_kernel(const float* src, const float* tgt, int B, long D, float* dist) {
    __shared__ float sa[OT_T][OT_K + 1], sb[OT_T][OT_K + 1];
    const int r = threadIdx.x >> 4, c = threadIdx.x & 15;
    const int i0 = blockIdx.y * OT_T, j0 = blockIdx.x * OT_T;
    float acc = 0.f;
    for (long k0 = 0; k0 < D; k0 += OT_K) {
        for (int e = threadIdx.x; e < OT_T * OT_K; e += 256) {
            const int rr = e / OT_K, kk = e % OT_K;
            const bool kin = k0 + kk < D;
            sa[rr][kk] = (kin && i0 + rr < B) ? src[(size_t)(i0 + rr) * D + k0 + kk] : 0.f;
            sb[rr][kk] = (kin && j0 + rr < B) ? tgt[(size_t)(j0 + rr) * D + k0 + kk] : 0.f;
        }
        __syncthreads();
#pragma unroll 16
        for (int kk = 0; kk < OT_K; ++kk) { const float d = sa[r][kk] - sb[c][kk]; acc += d * d; }
        __syncthreads();
    }
    if (i0 + r < B && j0 + c < B) dist[(size_t)(i0 + r) * B + j0 + c] = SQ ? ot_finite(acc) : sqrtf(acc);
}

// Small batches (the training step's 32 - 128 rows): a T x T tile per workgroup leaves 256 / T^2 threads per pair, which split the
// feature axis (lane-strided, coalesced) and meet in a fixed butterfly.  With 16 x 16 tiles a batch of 64 was 16 workgroups, each
// thread walking all D features alone: 234 us for 64 x 64 distances over 4096 features.
template <int T, bool SQ = false>
__global__ void __launch_bounds__(256) ot_dist_small_kernel(const float* src, const float* tgt, int B, long D, float* dist) {
    constexpr int KG = 256 / (T * T);
    const int pair = threadIdx.x / KG, kg = threadIdx.x % KG;
    const int i = blockIdx.y * T + pair / T, j = blockIdx.x * T + pair % T;
    const bool in = i < B && j < B;
    const float* a = src + (size_t)(in ? i : 0) * D;
    const float* b = tgt + (size_t)(in ? j : 0) * D;
    float acc = 0.f;
    for (long k = kg; k < D; k += KG) { const float d = a[k] - b[k]; acc += d * d; }
#pragma unroll
    for (int o = KG / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (in && kg == 0) dist[(size_t)i * B + j] = SQ ? ot_finite(acc) : sqrtf(acc);
}

// 1 block of 64 threads; B <= 4096.  LARGEST turns the comparison round: row by row the largest entry among the unused columns (first
// maximum), the sweep that turns a transport plan into a permutation (fc_ot_plan_pairing).
template <bool LARGEST = false>
__global__ void __launch_bounds__(64) ot_sweep_kernel(const float* dist, int B, long long* perm) {
    // the sweep is one dependent step per row; with the matrix in LDS (B <= 128) a step is an LDS read and six shuffles instead of a
    // round trip to memory (59 -> 15 us at B = 64)
    __shared__ float sd[128 * 128];
    const int lane = threadIdx.x, per = (B + 63) / 64;
    const bool staged = B <= 128;
    if (staged) {
        for (int e = lane; e < B * B; e += 64) sd[e] = dist[e];
        __syncthreads();
    }
    unsigned long long used = 0ull;
    for (int i = 0; i < B; ++i) {
        const float* row = staged ? sd + i * B : dist + (size_t)i * B;
        float best = LARGEST ? -INFINITY : INFINITY;
        int bj = 0x7fffffff;
        for (int q = 0; q < per; ++q) {
            const int j = q * 64 + lane;
            if (j < B && !((used >> q) & 1ull)) {
                const float v = row[j];
                if (LARGEST ? v > best : v < best) { best = v; bj = j; }   // ascending j per lane: keeps the first minimum
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o);
            const int oj = __shfl_xor(bj, o);
            if ((LARGEST ? ov > best : ov < best) || (ov == best && oj < bj)) { best = ov; bj = oj; }
        }
        if (bj == 0x7fffffff) {   // no finite minimum in this row (NaN / inf distances): take the first unused column, keep perm a permutation
            for (int q = 0; q < per; ++q) {
                const int j = q * 64 + lane;
                if (j < B && !((used >> q) & 1ull)) { bj = j; break; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { const int oj = __shfl_xor(bj, o); bj = oj < bj ? oj : bj; }
        }
        if ((bj & 63) == lane) used |= 1ull << (bj >> 6);
        if (lane == 0) perm[i] = bj;
    }
}

int ot_launch(const float* src, const float* tgt, int B, int64_t D, float* dist, int64_t* perm, hipStream_t s) {
    if (B < 1 || B > 4096) return fail(FC_E_SHAPE, "ot: batch must be in [1, 4096]");
    if (B <= 64) hipLaunchKernelGGL(ot_dist_small_kernel<4>, dim3(cdiv(B, 4), cdiv(B, 4)), dim3(256), 0, s, src, tgt, B, (long)D, dist);
    else if (B <= 128) hipLaunchKernelGGL(ot_dist_small_kernel<8>, dim3(cdiv(B, 8), cdiv(B, 8)), dim3(256), 0, s, src, tgt, B, (long)D, dist);
    else hipLaunchKernelGGL(ot_dist_kernel<false>, dim3(cdiv(B, OT_T), cdiv(B, OT_T)), dim3(256), 0, s, src, tgt, B, (long)D, dist);
    FC_HIP(hipGetLastError());
    hipLaunchKernelGGL(ot_sweep_kernel<false>, dim3(1), dim3(64), 0, s, dist, B, reinterpret_cast<long long*>(perm));
    FC_HIP(hipGetLastError());
    return FC_OK;
}

int ot_sweep_only_launch(const float* dist, int B, int64_t* perm, hipStream_t s) {
    if (B < 1 || B > 4096) return fail(FC_E_SHAPE, "ot: batch must be in [1, 4096]");
    hipLaunchKernelGGL(ot_sweep_kernel<false>, dim3(1), dim3(64), 0, s, dist, B, reinterpret_cast<long long*>(perm));
    FC_HIP(hipGetLastError());
    return FC_OK;
}

int ot_sweep_largest_launch(const float* plan, int B, int64_t* perm, hipStream_t s) {
    if (B < 1 || B > 4096) return fail(FC_E_SHAPE, "ot: batch must be in [1, 4096]");
    hipLaunchKernelGGL(ot_sweep_kernel<true>, dim3(1), dim3(64), 0, s, plan, B, reinterpret_cast<long long*>(perm));
    FC_HIP(hipGetLastError());
    return FC_OK;
}

// ---- exact pairing: linear sum assignment ------------------------------------------------------------------------------------
// Shortest augmenting paths (Jonker-Volgenant, as scipy's linear_sum_assignment) on c [B][B] fp32, duals in fp64.
//   start:    u_i = min_j c_ij, v = 0; row i takes its first-minimum column if no earlier row has it.
//   augment:  for every row the start left free, in ascending order: a Dijkstra over columns from that row -- minv_j the shortest
//             reduced-cost path to column j, way_j the row it came from -- until the nearest unvisited column is free; then the duals
//             move by (radius - minv) on the visited columns inside the radius and their rows (radius = the path length, but see
//             "Sentinels and the duals"), and the path's matches flip.
// Ties go to the lowest column (the lexicographic (value, index) butterfly of the sweep kernel), `<` keeps the first `way`.
// One wave64 because the algorithm is one dependent chain of argmins: column j lives in lane j % 64, register j / 64 (PER registers a
// lane), so a visit is PER row reads, PER fp64 updates and six shuffle steps, with no barrier inside it.  Row-indexed state (u, the two
// match tables, `way` for the walk) is in LDS; so is the matrix while 4 B^2 + 20 B bytes fit the 160 KB of a CDNA4 workgroup (B <= 192).
// Every loop has a trip count fixed by B: B start rows, at most B augmentations, at most B visits in one (each marks a new column
// and a free column exists while a row is free), at most B steps in the walk back.  All values compared are finite (ot_finite, fp64
// sums of at most 2B + 1 terms of magnitude <= FLT_MAX), so no input changes those counts.
//
// Sentinels and the duals.  A row of sentinels has u = FLT_MAX and reduced costs (c - u) - v = -v, formed c - u first so that they are
// exact whatever the path length: such a row is a row of equal costs, nothing of its scale reaches the other duals.  A sentinel
// COLUMN, or a lone sentinel entry, is different: a finite row is driven onto it only when nothing else is free, over a path of length
// ~FLT_MAX, and a dual update of that size would wipe the low bits of every visited dual (ulp(FLT_MAX) = 2^75 in fp64).  So the update's
// radius stops at the last visit whose path length is below OT_BIG = FLT_MAX / 2: columns and rows inside the radius move as usual (duals
// stay feasible, their matched pairs tight), what was reached beyond it keeps its duals.  The permutation is not affected by this (the
// search and the walk are unchanged); u_i + v_j = c_ij then holds on the pairs matched inside the radius, not on a pair that holds a
// sentinel or was reached over one.  Finite entries of magnitude >= FLT_MAX / 4 in a caller's matrix count as that scale too.
constexpr int OT_LDS_B = 192;
constexpr double OT_BIG = 0.5 * (double)FLT_MAX;

template <int PER, bool STAGED>
__global__ void __launch_bounds__(64) ot_assign_kernel(const float* cost, int B, long long* perm, double* duals) {
    extern __shared__ double ot_smem[];
    double* u = ot_smem;                                  // [B]
    int* col4row = reinterpret_cast<int*>(u + B);         // [B] column matched to row i, -1 = free
    int* row4col = col4row + B;                           // [B] row matched to column j, -1 = free
    int* way = row4col + B;                               // [B] predecessor row of column j on the current shortest-path tree
    float* sc = reinterpret_cast<float*>(way + B);        // [B][B] when STAGED
    const int lane = threadIdx.x;
    if (STAGED)
        for (int e = lane; e < B * B; e += 64) sc[e] = ot_finite(cost[e]);
    for (int i = lane; i < B; i += 64) { col4row[i] = -1; row4col[i] = -1; }
    __syncthreads();
    auto at = [&](int i, int j) -> float { return STAGED ? sc[i * B + j] : ot_finite(cost[(size_t)i * B + j]); };

    // start: row minima, next row prefetched while the current one is reduced
    float nxt[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) { const int j = q * 64 + lane; nxt[q] = j < B ? at(0, j) : FLT_MAX; }
    for (int i = 0; i < B; ++i) {
        float best = INFINITY;
        int bj = 0x7fffffff;
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int j = q * 64 + lane;
            const float c = nxt[q];
            if (j < B && c < best) { best = c; bj = j; }
            if (i + 1 < B) nxt[q] = j < B ? at(i + 1, j) : FLT_MAX;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o);
            const int oj = __shfl_xor(bj, o);
            if (ov < best || (ov == best && oj < bj)) { best = ov; bj = oj; }
        }
        if (lane == 0) {
            u[i] = (double)best;
            if (bj < B && row4col[bj] < 0) { row4col[bj] = i; col4row[i] = bj; }
        }
    }

    double v[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) v[q] = 0.0;

    for (int cur = 0; cur < B; ++cur) {
        __syncthreads();
        if (__builtin_amdgcn_readfirstlane(col4row[cur]) >= 0) continue;
        double minv[PER];
        int wy[PER];
#pragma unroll
        for (int q = 0; q < PER; ++q) { minv[q] = INFINITY; wy[q] = -1; }
        unsigned vis = 0u;
        int i = cur, sink = -1;
        double path = 0.0, radius = 0.0;
        for (int it = 0; it < B; ++it) {
            const double ui = u[i];
            double best = INFINITY;
            int bj = 0x7fffffff;
#pragma unroll
            for (int q = 0; q < PER; ++q) {
                const int j = q * 64 + lane;
                if (j < B && !((vis >> q) & 1u)) {
                    const double r = path + (((double)at(i, j) - ui) - v[q]);   // c - u first: exact (zero) on a row of sentinels, whatever the path
                    if (r < minv[q]) { minv[q] = r; wy[q] = i; }
                    if (minv[q] < best) { best = minv[q]; bj = j; }   // ascending j per lane: keeps the first minimum
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ov = __shfl_xor(best, o);
                const int oj = __shfl_xor(bj, o);
                if (ov < best || (ov == best && oj < bj)) { best = ov; bj = oj; }
            }
            if (bj >= B) break;   // unreachable: an unvisited column exists and its minv is finite
            path = best;
            if (best < OT_BIG) radius = best;   // the dual update stops before a hop of sentinel scale
            if ((bj & 63) == lane) vis |= 1u << (bj >> 6);
            const int r4 = __builtin_amdgcn_readfirstlane(row4col[bj]);
            if (r4 < 0) { sink = bj; break; }
            i = r4;
        }
        if (sink < 0) continue;
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int j = q * 64 + lane;
            if (j < B) {
                way[j] = wy[q];
                const double d = radius - minv[q];
                if (((vis >> q) & 1u) && d > 0.0) {
                    v[q] -= d;
                    const int r = row4col[j];
                    if (r >= 0) u[r] += d;   // the visited columns' rows are distinct
                }
            }
        }
        if (lane == 0) u[cur] += radius;
        __syncthreads();
        if (lane == 0) {
            int j = sink;
            for (int k = 0; k < B; ++k) {
                const int r = way[j];
                if (r < 0) break;   // unreachable: every column on the path was reached from a row
                row4col[j] = r;
                const int t = col4row[r];
                col4row[r] = j;
                j = t;
                if (r == cur) break;
            }
        }
    }
    __syncthreads();
    for (int i = lane; i < B; i += 64) {
        perm[i] = col4row[i];
        if (duals) duals[i] = u[i];
    }
    if (duals) {
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int j = q * 64 + lane;
            if (j < B) duals[B + j] = v[q];
        }
    }
}

template <int PER, bool STAGED>
static int ot_assign_run(const float* cost, int B, int64_t* perm, double* duals, hipStream_t s) {
    const size_t lds = (size_t)B * 20 + (STAGED ? (size_t)B * B * 4 : 0);
    if (lds > 64 * 1024)   // only B in 129..192; per launch, the attribute belongs to the current device
        FC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&ot_assign_kernel<PER, STAGED>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   160 * 1024));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(ot_assign_kernel<PER, STAGED>), dim3(1), dim3(64), lds, s, cost, B, reinterpret_cast<long long*>(perm),
                       duals);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

int ot_assign_launch(const float* cost, int B, int64_t* perm, double* duals, hipStream_t s) {
    if (B < 1 || B > 1024) return fail(FC_E_SHAPE, "ot (exact): batch must be in [1, 1024]");
    if (B <= 64) return ot_assign_run<1, true>(cost, B, perm, duals, s);
    if (B <= 128) return ot_assign_run<2, true>(cost, B, perm, duals, s);
    if (B <= OT_LDS_B) return ot_assign_run<3, true>(cost, B, perm, duals, s);
    if (B <= 256) return ot_assign_run<4, false>(cost, B, perm, duals, s);
    if (B <= 512) return ot_assign_run<8, false>(cost, B, perm, duals, s);
    return ot_assign_run<16, false>(cost, B, perm, duals, s);
}

int ot_sqdist_launch(const float* src, const float* tgt, int B, int64_t D, float* cost, hipStream_t s) {
    if (B <= 64)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(ot_dist_small_kernel<4, true>), dim3(cdiv(B, 4), cdiv(B, 4)), dim3(256), 0, s, src, tgt, B, (long)D, cost);
    else if (B <= 128)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(ot_dist_small_kernel<8, true>), dim3(cdiv(B, 8), cdiv(B, 8)), dim3(256), 0, s, src, tgt, B, (long)D, cost);
    else
        hipLaunchKernelGGL(ot_dist_kernel<true>, dim3(cdiv(B, OT_T), cdiv(B, OT_T)), dim3(256), 0, s, src, tgt, B, (long)D, cost);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

int ot_exact_launch(const float* src, const float* tgt, int B, int64_t D, float* cost, int64_t* perm, double* duals, hipStream_t s) {
    if (B < 1 || B > 1024) return fail(FC_E_SHAPE, "ot (exact): batch must be in [1, 1024]");
    FC_TRY(ot_sqdist_launch(src, tgt, B, D, cost, s));
    return ot_assign_launch(cost, B, perm, duals, s);
}

}  // namespace fc
