// Entropic (Sinkhorn) transport plans between two uniform mini-batches, and what is done with a plan: sampling index pairs from it with
// replacement (torchcfm's OTPlanSampler.sample_map) and turning it into a permutation (upstream's compute_ot_pairing_vanilla sweep).
//
// The solver is POT's sinkhorn_knopp restated in the log domain.  Kernel-form Sinkhorn builds K = exp(-C / reg); with squared distances
// around 8000 (4 x 32 x 32 latents) and reg = 0.05 every entry of K is exp(-160000) = 0, the scalings divide by zero and torchcfm falls
// back to the uniform plan.  In the log domain nothing underflows that matters:
//     start   f = g = reg log(1/B)
//     repeat  g_j = reg (log(1/B) - LSE_i((f_i - C_ij) / reg))         (columns)
//             f_i = reg (log(1/B) - LSE_j((g_j - C_ij) / reg))         (rows)
//             after every 10th iteration: err = | colsum(P) - 1/B |_2,  P_ij = exp((f_i + g_j - C_ij) / reg);  stop when err < stop_thr
// The last update is always the row half, so the plan's row sums are 1/B to rounding and err measures the columns alone.
//
// How a log-sum-exp is formed, and the sentinel.  The maximum is taken of the numerators, m = max_j (g_j - C_ij), then
// s = sum_j exp(((g_j - C_ij) - m) / reg) and f_i = reg (log(1/B) - log s) - m: the same value as the line above.  A row of FLT_MAX
// sentinels (a non-finite source sample) gets m = -FLT_MAX, s = B and f_i = FLT_MAX exactly; a sentinel column (a non-finite target
// sample) gets g_j = FLT_MAX the same way.  The exponent of a plan entry is therefore formed as (hi - C_ij) + lo with hi the larger of
// f_i and g_j (skp_arg): on a sentinel row that is (FLT_MAX - FLT_MAX) + g_j = g_j, on a sentinel column f_i, entries exp(g_j / reg) or
// exp(f_i / reg) <= 1/B; a fixed order gives (-FLT_MAX) + FLT_MAX = 0 -- a column of ones -- on one of the two, and f + g first gives
// exp(+-2^75 / reg).  In the halves the sentinel line enters the other side's sums with numerator 0, as a line of zero cost and zero
// potential would, so it soaks up mass; its own marginal is not enforced by its own update (it is 1/B at convergence only because all the
// other lines' are and the total is 1).  A sentinel row AND column: the row takes FLT_MAX first, the column's potential stays small.
// Division by reg is a multiplication by the fp64 1 / reg (one ulp of the exponent's argument, 1e-14 relative at arguments of 100).
//
// Shape: ONE launch, one workgroup of up to 16 waves, for the reason ot_assign_kernel is one wave: an iteration is two dependent halves,
// a grid of workgroups would need a grid barrier between them and a launch per half is 2000 launches.  A wave owns a row (a column on the
// g half) and its lanes stride the other index; max and sum meet in xor butterflies, whose result is the same bits in every lane.  The
// potentials and every accumulation are fp64 (potentials reach max(C) while reg is 1e-2: sinkhorn.hip has the argument); the matrix
// stays fp32 and sits in LDS while 4 B (B|1) + 24 B + 16 bytes fit the 160 KB of a CDNA4 workgroup (B <= 192), with an odd row pitch so
// that the column half, whose lanes walk down a column, touches 64 different banks; above that it is read from memory (L2 resident:
// 4 MB at B = 1024), the column half with a stride of one row.  Every loop has a trip count fixed by B and max_iter; the stop decision is
// written to LDS by one lane and read by all threads after a barrier, so every barrier is reached by the whole workgroup.
//
// Cost per iteration: 2 B^2 fp64 exponentials (plus B^2 on every 10th and B^2 for the plan), ~40 fp64 operations each at 8 lanes per
// clock and SIMD: 2 B^2 * 40 / 32 clocks = 65 us at B = 256 on the one CU as a floor.  Measured there: 116 us per iteration (1.16 ms for
// 10 iterations, one check and the plan write, i.e. ~50 us per B^2 exponentials -- the max pass, the log and, above B = 192, the column
// half's reads with a stride of one row come on top of the floor); 36 us at B = 128, 15 us at B = 64, where a row is one element per lane
// and the butterflies' latency is what an iteration costs.  Bound by one CU's fp64 rate, not by memory bandwidth.
//
// Run time is the caller's to bound: max_iter up to 10000 is accepted at every B.  Scaling the measured figure by B^2, an iteration at
// B = 1024 is about 2 ms, so POT's default of 1000 iterations without convergence is 2 s and max_iter = 10000 is 20 s of one CU, with the
// stream behind it waiting.  The training path uses batches of 32 - 256 and the normalised cost, which converged in 10 - 20 iterations.
#include <float.h>

#include "common.h"
#include "philox.h"

namespace fc {

constexpr int SKP_LDS_B = 192;

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the exponent's numerator (f_i + g_j - c), the larger potential meeting the cost first ("the sentinel" above)
__device__ __forceinline__ double skp_arg(double fi, double gj, double c) { return fi >= gj ? (fi - c) + gj : (gj - c) + fi; }

// info: {iterations run, converged (0 / 1), err at the last check}
template <bool STAGED>
__global__ void __launch_bounds__(1024) ot_sinkhorn_kernel(const float* cost, int B, double reg, double rinv, int max_iter, double stop_thr,
                                                           float* plan, double* duals, double* info) {
    extern __shared__ double skp_smem[];
    double* f = skp_smem;                               // [B]
    double* g = f + B;                                  // [B]
    double* res = g + B;                                // [B] colsum - 1/B at a check; res[B]: err
    int* stop = reinterpret_cast<int*>(res + B + 1);    // [2]
    float* sc = reinterpret_cast<float*>(stop + 2);     // [B][P] when STAGED
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const int P = STAGED ? (B | 1) : B;
    if (STAGED)
        for (int e = tid; e < B * B; e += blockDim.x) sc[(e / B) * P + e % B] = ot_finite(cost[e]);
    const double lb = -log((double)B), inv_b = 1.0 / (double)B;
    for (int i = tid; i < B; i += blockDim.x) { f[i] = reg * lb; g[i] = reg * lb; }
    if (tid == 0) { stop[0] = 0; res[B] = INFINITY; }
    __syncthreads();
    auto at = [&](int i, int j) -> double { return (double)(STAGED ? sc[i * P + j] : ot_finite(cost[(size_t)i * B + j])); };

    int iters = 0;
    for (int it = 1; it <= max_iter; ++it) {
        for (int j = wave; j < B; j += nw) {            // columns
            double m = -INFINITY;
            for (int i = lane; i < B; i += 64) m = fmax(m, f[i] - at(i, j));
            m = wave_max(m);
            double s = 0.0;
            for (int i = lane; i < B; i += 64) s += exp(((f[i] - at(i, j)) - m) * rinv);
            s = wave_sum(s);
            if (lane == 0) g[j] = reg * (lb - log(s)) - m;
        }
        __syncthreads();
        for (int i = wave; i < B; i += nw) {            // rows
            double m = -INFINITY;
            for (int j = lane; j < B; j += 64) m = fmax(m, g[j] - at(i, j));
            m = wave_max(m);
            double s = 0.0;
            for (int j = lane; j < B; j += 64) s += exp(((g[j] - at(i, j)) - m) * rinv);
            s = wave_sum(s);
            if (lane == 0) f[i] = reg * (lb - log(s)) - m;
        }
        __syncthreads();
        iters = it;
        if (it % 10 == 0) {                             // uniform: `it` is the same in every thread
            for (int j = wave; j < B; j += nw) {
                const double gj = g[j];
                double s = 0.0;
                for (int i = lane; i < B; i += 64) s += exp(skp_arg(f[i], gj, at(i, j)) * rinv);
                s = wave_sum(s);
                if (lane == 0) res[j] = s - inv_b;
            }
            __syncthreads();
            if (wave == 0) {
                double a = 0.0;
                for (int j = lane; j < B; j += 64) a += res[j] * res[j];
                a = wave_sum(a);
                if (lane == 0) { const double err = sqrt(a); res[B] = err; stop[0] = err < stop_thr ? 1 : 0; }
            }
            __syncthreads();
            if (stop[0]) break;                         // the same word in every thread
        }
    }
    for (int e = tid; e < B * B; e += blockDim.x) {
        const int i = e / B, j = e % B;
        plan[e] = (float)exp(skp_arg(f[i], g[j], at(i, j)) * rinv);
    }
    for (int i = tid; i < B; i += blockDim.x) { duals[i] = f[i]; duals[B + i] = g[i]; }
    if (tid == 0) { info[0] = (double)iters; info[1] = (double)stop[0]; info[2] = res[B]; }
}

int ot_sinkhorn_launch(const float* cost, int B, double reg, int max_iter, double stop_thr, float* plan, double* duals, double* info,
                       hipStream_t s) {
    if (B < 1 || B > 1024) return fail(FC_E_SHAPE, "ot (sinkhorn): batch must be in [1, 1024]");
    if (!(reg > 0.0) || !(reg <= DBL_MAX)) return fail(FC_E_ARG, "ot (sinkhorn): reg must be positive and finite");
    if (!(stop_thr >= 0.0)) return fail(FC_E_ARG, "ot (sinkhorn): stop_thr must be >= 0");
    if (max_iter < 1 || max_iter > 10000) return fail(FC_E_ARG, "ot (sinkhorn): max_iter must be in [1, 10000]");
    max_iter = (max_iter + 9) / 10 * 10;                 // the stopping rule looks at every 10th iteration
    const bool staged = B <= SKP_LDS_B;
    const size_t lds = (size_t)(3 * B + 1) * 8 + 8 + (staged ? (size_t)B * (B | 1) * 4 : 0);
    const int threads = 64 * (B < 16 ? B : 16);
    const double rinv = 1.0 / reg;
    if (staged) {
        if (lds > 64 * 1024)   // per launch, the attribute belongs to the current device
            FC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&ot_sinkhorn_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       160 * 1024));
        hipLaunchKernelGGL(ot_sinkhorn_kernel<true>, dim3(1), dim3(threads), lds, s, cost, B, reg, rinv, max_iter, stop_thr, plan, duals, info);
    } else {
        hipLaunchKernelGGL(ot_sinkhorn_kernel<false>, dim3(1), dim3(threads), lds, s, cost, B, reg, rinv, max_iter, stop_thr, plan, duals, info);
    }
    FC_HIP(hipGetLastError());
    return FC_OK;
}

// torchcfm's normalize_cost: the matrix divided by its largest entry, in place.  Sentinels (FLT_MAX) neither count as the maximum nor are
// divided; an all-zero matrix stays as it is.  1 block of 1024 threads.
__global__ void __launch_bounds__(1024) ot_normalize_kernel(float* cost, int n) {
    __shared__ float part[16];
    float m = 0.f;
    for (int e = threadIdx.x; e < n; e += 1024) { const float c = cost[e]; if (c < FLT_MAX) m = fmaxf(m, c); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    m = part[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) m = fmaxf(m, part[w]);
    if (!(m > 0.f)) return;                              // uniform
    for (int e = threadIdx.x; e < n; e += 1024) { const float c = cost[e]; if (c < FLT_MAX) cost[e] = c / m; }
}

int ot_normalize_launch(float* cost, int B, hipStream_t s) {
    hipLaunchKernelGGL(ot_normalize_kernel, dim3(1), dim3(1024), 0, s, cost, B * B);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

// ---- sampling pairs from a plan -----------------------------------------------------------------------------------------------
// Pair k of draw `draw` is the cell of the plan, read as a categorical over its B^2 cells in row-major order, that inverts
//     u_k = ((r0 >> 5) 2^26 + (r1 >> 6) + 0.5) 2^-53,     (r0, r1, ., .) = philox4x32_10(counter (k, draw, 0x4F54504C, 0xFFFFFFFF), key = seed)
// (a 53-bit uniform; the one value 2^53 - 1/2 rounds to u = 1, which the clamp below takes).  The search is two-level, in fp64, every sum
// sequential in ascending index so that a host restatement forms the same bits: R_i = the running sum of the row sums, t = u R_{B-1},
// the row is the number of R_i <= t (clamped to B - 1), then t' = t - R_{row-1} and the column is the first j at which the row's running
// sum exceeds t' (B - 1 if none does).  Each workgroup forms R for itself in LDS (B^2 reads; no workspace, no second launch).
// A plan whose total is not positive and finite gives the identity pairs (k mod B, k mod B) and sets *info = 1 (never cleared here).
__global__ void __launch_bounds__(256) ot_sample_kernel(const float* plan, int B, int n, unsigned long long seed, unsigned draw,
                                                        long long* i_out, long long* j_out, int* info) {
    extern __shared__ double rs[];                      // [B]
    __shared__ int bad;
    for (int r = threadIdx.x; r < B; r += 256) {
        const float* row = plan + (size_t)r * B;
        double a = 0.0;
        for (int j = 0; j < B; ++j) a += (double)row[j];
        rs[r] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0;
        for (int r = 0; r < B; ++r) { a += rs[r]; rs[r] = a; }
        bad = !(a > 0.0 && a <= DBL_MAX);
        if (bad && info && blockIdx.x == 0) *info = 1;
    }
    __syncthreads();
    const double total = rs[B - 1];
    for (int k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256) {
        if (bad) { i_out[k] = k % B; j_out[k] = k % B; continue; }
        unsigned r[4];
        philox4x32_10((unsigned)k, draw, 0x4F54504Cu, 0xFFFFFFFFu, (unsigned)seed, (unsigned)(seed >> 32), r);
        const double u = ((double)(r[0] >> 5) * 67108864.0 + (double)(r[1] >> 6) + 0.5) * 1.1102230246251565e-16;   // 2^-53
        const double t = u * total;
        int lo = 0, hi = B;
        for (int st = 0; st < 11; ++st) {               // B <= 1024: the interval is empty after at most 11 halvings
            if (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (rs[mid] <= t) lo = mid + 1; else hi = mid;
            }
        }
        const int row = lo < B ? lo : B - 1;
        const double tp = t - (row > 0 ? rs[row - 1] : 0.0);
        const float* pr = plan + (size_t)row * B;
        int col = B - 1;
        double a = 0.0;
        for (int j = 0; j < B; ++j) {
            a += (double)pr[j];
            if (a > tp) { col = j; break; }
        }
        i_out[k] = row; j_out[k] = col;
    }
}

int ot_sample_plan_launch(const float* plan, int B, int n_pairs, uint64_t seed, uint32_t draw, int64_t* i_out, int64_t* j_out, int* info,
                          hipStream_t s) {
    if (B < 1 || B > 1024) return fail(FC_E_SHAPE, "ot (sample): batch must be in [1, 1024]");
    if (n_pairs < 1 || n_pairs > 65536) return fail(FC_E_SHAPE, "ot (sample): n_pairs must be in [1, 65536]");
    const int blocks = cdiv(n_pairs, 256) < 64 ? cdiv(n_pairs, 256) : 64;
    hipLaunchKernelGGL(ot_sample_kernel, dim3(blocks), dim3(256), (size_t)B * 8, s, plan, B, n_pairs, (unsigned long long)seed, (unsigned)draw,
                       reinterpret_cast<long long*>(i_out), reinterpret_cast<long long*>(j_out), info);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

}  // namespace fc
