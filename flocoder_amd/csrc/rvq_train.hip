// Fitting the residual quantiser's codebooks without gradients (vector_quantize_pytorch's EuclideanCodebook as VQVAE configures it,
// codecs.py:456-467: k-means initialisation, EMA updates, dead-code expiry).  THIRD-PARTY ALGORITHM, PARITY UNPINNED, as rvq.hip; the
// definition is DESIGN.md section 4 "Codebook fitting" and flocoder_amd/noise.py (codebook_*), the fp64 restatement tests/rvq_fit_ref.py.
//
// Launches (all on the caller's stream, nothing allocated, no host read):
//   rvq_bound_kernel    max|z| and max|E_l| as integer atomic maxima of the fp32 bit patterns -> the fixed-point scale below
//   rvq_assign_kernel   one thread per latent vector walks levels 0..last with rvq_nearest (rvq_dev.h, the search of fc_rvq_quantize) and,
//                       from level `first` on, adds to the level's counts, sums and commitment sum
//   rvq_kmeans_kernel   mean_k = S_k / n_k (an empty cluster keeps its mean), the iteration's objective
//   rvq_ema_kernel      one workgroup per level: cluster_size, embed_avg, smoothed codebook, dead-code expiry, the level's loss
//   rvq_seed_kernel     drawn residual vectors into a level's code slots
//   codebook_draws_kernel   the draw field by itself
//
// ACCUMULATION, reproducible run to run: counts are 32-bit integer atomics; the sums S_k are 64-bit integer atomics on fixed-point values
// q = rint(r 2^s).  Integer addition is associative, so the order in which vectors arrive does not reach the result.  With
// M = max|z| + sum_{l' < last} max|E_l'| (every accumulated residual obeys |r| <= M up to the fp32 rounding of its L subtractions, a factor
// 1 + L 2^-24) and e the exponent with M < 2^e, s = 38 - e: |q| < 2^38 and a sum of N <= 2^24 of them stays below 2^62, inside int64 with a
// factor two to spare.  One conversion errs by at most half a unit, 2^-(s+1) = 2^(e-39) <= M 2^-38, so
//     |S_k(device) - S_k(exact)| <= n_k 2^(e-39)      and the mean S_k / n_k by 2^(e-39) <= M 2^-38
// (an fp32 ulp of a value of size M is M 2^-23: the fixed point costs 2^-15 of it).  The commitment sum is fp64 throughout: per vector in
// index order of d, per wave by a fixed butterfly, one slot per wave, the slots summed in a fixed order by the finishing kernel; its
// relative error is at most (D + 6 + log2(slots)) 2^-53 plus nothing that depends on the run.
#include "common.h"
#include "philox.h"
#include "rvq_dev.h"

namespace fc {

constexpr long RVQ_MAX_N = 1l << 24;

// ---- draws: a keyed bijection of [0, 2^b) cycle-walked into [0, n); noise.py codebook_draws is the host form ---------------------------
__device__ __forceinline__ unsigned codebook_draw(unsigned long long seed, unsigned level, unsigned draw, unsigned slot, unsigned n) {
    const unsigned long long key = seed + FC_CODEBOOK_KEY_OFFSET;
    unsigned m[4], a[4];
    philox4x32_10(0u, draw, level, n, (unsigned)key, (unsigned)(key >> 32), m);
    philox4x32_10(1u, draw, level, n, (unsigned)key, (unsigned)(key >> 32), a);
    const int b = n <= 2u ? 1 : 32 - __clz(n - 1u);      // smallest b >= 1 with 2^b >= n
    const unsigned mask = (1u << b) - 1u;
    const int sh = (b + 1) / 2;
    unsigned x = slot % n;
    do {                                                  // a permutation's cycle through x < n returns below n: the walk ends
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            x = (x * (m[r] | 1u) + a[r]) & mask;          // odd multiplier: a bijection of the b-bit words
            x ^= x >> sh;                                 // and so is the xor with the upper half
        }
    } while (x >= n);
    return x;
}

__global__ void __launch_bounds__(256) codebook_draws_kernel(int64_t* out, unsigned long long seed, unsigned level, unsigned draw, unsigned n, long count) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j < count) out[j] = codebook_draw(seed, level, draw, (unsigned)(j % n), n);
}

// ---- workspace --------------------------------------------------------------------------------------------------------------------------
struct RvqWs {
    unsigned* maxbits;              // [1 + L]: bit patterns of max|z|, max|E_l|
    unsigned* counts;               // [L][K]
    unsigned long long* sums;       // [L][K][D] fixed point
    double* part;                   // [L][4 * grid]: one commitment partial per wave
    float* cb0;                     // [L][K][D]: the codebooks a training step assigned against
    size_t zero_bytes, acc_off, bytes;
    int grid;
};

static inline size_t up64(size_t v) { return (v + 63) / 64 * 64; }

static RvqWs ws_layout(void* base, long n, int D, int K, int L) {
    RvqWs w;
    char* p = static_cast<char*>(base);
    w.grid = (int)((n + 255) / 256);
    size_t o = 0;
    w.maxbits = reinterpret_cast<unsigned*>(p + o); o += up64((size_t)(1 + L) * 4);
    w.acc_off = o;
    w.counts = reinterpret_cast<unsigned*>(p + o); o += up64((size_t)L * K * 4);
    w.sums = reinterpret_cast<unsigned long long*>(p + o); o += up64((size_t)L * K * D * 8);
    w.zero_bytes = o;
    w.part = reinterpret_cast<double*>(p + o); o += up64((size_t)L * 4 * w.grid * 8);
    w.cb0 = reinterpret_cast<float*>(p + o); o += up64((size_t)L * K * D * 4);
    w.bytes = o;
    return w;
}

// s of the header comment from the maxima of levels < nlev
__device__ __forceinline__ int rvq_fix_shift(const unsigned* maxbits, int nlev) {
    double m = (double)__uint_as_float(maxbits[0]);
    for (int l = 0; l < nlev; ++l) m += (double)__uint_as_float(maxbits[1 + l]);
    int e = 0;
    if (m > 0.0 && m < 1e38) frexp(m, &e);               // m = f 2^e with f in [0.5, 1): m < 2^e
    else if (!(m < 1e38)) e = 128;                        // inf / NaN input: nothing below is meaningful, and nothing is out of bounds
    e = e < -64 ? -64 : e;
    return 38 - e;
}

__global__ void __launch_bounds__(256) rvq_bound_kernel(const float* z, long nz, const float* cb, int KD, int nlev, unsigned* maxbits) {
    const int lane = threadIdx.x & 63;
    unsigned mb = 0;                                     // unsigned order of |x|'s bits = order of |x|, and a NaN sorts above everything
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nz; i += (long)gridDim.x * 256) {
        const unsigned v = __float_as_uint(fabsf(z[i]));
        mb = v > mb ? v : mb;
    }
    for (int o = 32; o > 0; o >>= 1) { const unsigned t = __shfl_xor(mb, o); mb = t > mb ? t : mb; }
    if (lane == 0 && mb) atomicMax(&maxbits[0], mb);
    for (int l = blockIdx.x; l < nlev; l += gridDim.x) {
        unsigned e = 0;
        for (int i = threadIdx.x; i < KD; i += 256) { const unsigned v = __float_as_uint(fabsf(cb[(size_t)l * KD + i])); e = v > e ? v : e; }
        for (int o = 32; o > 0; o >>= 1) { const unsigned t = __shfl_xor(e, o); e = t > e ? t : e; }
        if (lane == 0 && e) atomicMax(&maxbits[1 + l], e);
    }
}

// grid (ceil(N/256)), LDS (last+1)*K*D floats.  idx [N][L] or null; zq written when non-null (the caller passes it with last = L-1)
__global__ void __launch_bounds__(256) rvq_assign_kernel(const float* z, const float* cb, float* zq, int64_t* idx, RvqWs w, int first, int last,
                                                         int B, int D, int HW, int K, int L, int keep_cb) {
    extern __shared__ __attribute__((aligned(16))) float cs[];   // [last+1][K][D]
    for (int i = threadIdx.x; i < (last + 1) * K * D; i += 256) {
        const float v = cb[i];
        cs[i] = v;
        if (keep_cb && blockIdx.x == 0) w.cb0[i] = v;
    }
    __syncthreads();
    const int s = rvq_fix_shift(w.maxbits, last);
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    const bool valid = n < (long)B * HW;
    const int b = valid ? (int)(n / HW) : 0, p = valid ? (int)(n % HW) : 0;
    const float* zp = z + (size_t)b * D * HW + p;
    float r[RVQ_MAXD], q[RVQ_MAXD];
#pragma unroll
    for (int d = 0; d < RVQ_MAXD; ++d) { r[d] = (valid && d < D) ? zp[(size_t)d * HW] : 0.f; q[d] = 0.f; }
    for (int l = 0; l <= last; ++l) {
        const float* cl = cs + (size_t)l * K * D;
        const int bi = rvq_nearest(r, cl, K, D);
        if (l >= first) {
            double dist = 0.0;
#pragma unroll
            for (int d = 0; d < RVQ_MAXD; ++d)
                if (d < D) { const double t = (double)r[d] - (double)cl[bi * D + d]; dist += t * t; }
            if (valid) {
                atomicAdd(&w.counts[(size_t)l * K + bi], 1u);
                unsigned long long* sp = w.sums + ((size_t)l * K + bi) * D;
#pragma unroll
                for (int d = 0; d < RVQ_MAXD; ++d)
                    if (d < D) atomicAdd(&sp[d], (unsigned long long)__double2ll_rn(scalbn((double)r[d], s)));
            } else {
                dist = 0.0;
            }
            for (int o = 32; o > 0; o >>= 1) dist += __shfl_xor(dist, o);
            if ((threadIdx.x & 63) == 0) w.part[((size_t)l * gridDim.x + blockIdx.x) * 4 + (threadIdx.x >> 6)] = dist;
        }
#pragma unroll
        for (int d = 0; d < RVQ_MAXD; ++d)
            if (d < D) { const float e = cl[bi * D + d]; r[d] -= e; q[d] += e; }
        if (valid && idx) idx[n * L + l] = bi;
    }
    if (valid && zq) {
        float* qp = zq + (size_t)b * D * HW + p;
#pragma unroll
        for (int d = 0; d < RVQ_MAXD; ++d)
            if (d < D) qp[(size_t)d * HW] = q[d];
    }
}

// the `slots` partials of level l in a fixed order: thread t its strided share in index order, then a fixed tree.  All 256 threads call it.
__device__ __forceinline__ double rvq_part_sum(const double* part, int slots, double* red) {
    double p = 0.0;
    for (int j = threadIdx.x; j < slots; j += 256) p += part[j];
    red[threadIdx.x] = p;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

// residual of vector n entering level l: z minus the chosen codewords of levels < l, in rvq_kernel's order.  idx null: the search is redone.
__device__ __forceinline__ void rvq_residual(float (&r)[RVQ_MAXD], const float* z, const float* cb, const int64_t* idx, long n, int l, int D, int HW,
                                             int K, int L) {
    const int b = (int)(n / HW), p = (int)(n % HW);
#pragma unroll
    for (int d = 0; d < RVQ_MAXD; ++d) r[d] = d < D ? z[((size_t)b * D + d) * HW + p] : 0.f;
    for (int j = 0; j < l; ++j) {
        const float* cl = cb + (size_t)j * K * D;
        int bi = idx ? (int)idx[n * L + j] : rvq_nearest(r, cl, K, D);
        bi = bi < 0 ? 0 : (bi >= K ? K - 1 : bi);
#pragma unroll
        for (int d = 0; d < RVQ_MAXD; ++d)
            if (d < D) r[d] -= cl[bi * D + d];
    }
}

// grid (ceil(K*D/256)); block 0 also sums the objective
__global__ void __launch_bounds__(256) rvq_kmeans_kernel(float* cb, RvqWs w, int l, int K, int D, float* cs_out, float* ea_out, double* obj_out) {
    __shared__ double red[256];
    const int s = rvq_fix_shift(w.maxbits, l);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < K * D) {
        const int k = i / D;
        const unsigned n = w.counts[(size_t)l * K + k];
        float* e = cb + (size_t)l * K * D + i;
        if (n) *e = (float)(scalbn((double)(long long)w.sums[(size_t)l * K * D + i], -s) / (double)n);
        if (cs_out) {
            ea_out[i] = *e * (float)n;
            if (i == k * D) cs_out[k] = (float)n;
        }
    }
    if (blockIdx.x == 0 && obj_out) {
        const double t = rvq_part_sum(w.part + (size_t)l * 4 * w.grid, 4 * w.grid, red);
        if (threadIdx.x == 0) *obj_out = t;
    }
}

// grid (L), LDS K floats
__global__ void __launch_bounds__(256) rvq_ema_kernel(const float* z, float* cb, float* cs, float* ea, const int64_t* idx, RvqWs w, float* losses,
                                                      int* expired, int B, int D, int HW, int K, int L, double decay, double cweight, float thr,
                                                      unsigned long long seed, unsigned draw) {
    extern __shared__ __attribute__((aligned(16))) float csn[];  // [K]: the updated cluster sizes
    __shared__ double red[256];
    __shared__ double tot;
    __shared__ int scan[257];
    const int l = blockIdx.x, t = threadIdx.x;
    const int s = rvq_fix_shift(w.maxbits, L - 1);
    const double om = 1.0 - decay;
    const long N = (long)B * HW;
    cb += (size_t)l * K * D; cs += (size_t)l * K; ea += (size_t)l * K * D;
    const unsigned* cnt = w.counts + (size_t)l * K;
    const unsigned long long* sums = w.sums + (size_t)l * K * D;
    for (int k = t; k < K; k += 256) {
        const double c = (double)cs[k];
        const float v = (float)(c + om * ((double)cnt[k] - c));
        csn[k] = v;
        cs[k] = v;
    }
    const double csum = rvq_part_sum(w.part + (size_t)l * 4 * w.grid, 4 * w.grid, red);   // (its barriers also publish csn)
    if (t == 0) {
        losses[l] = (float)(cweight * csum / ((double)N * (double)D));
        double a = 0.0;
#pragma unroll 8
        for (int k = 0; k < K; ++k) a += (double)csn[k];     // in index order
        tot = a;
    }
    __syncthreads();
    const double T = tot, den = T + (double)K * 1e-5;
    for (int i = t; i < K * D; i += 256) {
        const int k = i / D;
        const double A = (double)ea[i];
        const float a = (float)(A + om * (scalbn((double)(long long)sums[i], -s) - A));
        ea[i] = a;
        cb[i] = (float)((double)a / (((double)csn[k] + 1e-5) / den * T));
    }
    if (!(thr > 0.f)) {
        if (t == 0) expired[l] = 0;
        return;
    }
    __syncthreads();
    const int per = (K + 255) / 256, k0 = t * per, k1 = k0 + per < K ? k0 + per : K;
    int c = 0;
    for (int k = k0; k < k1; ++k) c += csn[k] < thr;
    scan[t] = c;
    __syncthreads();
    if (t == 0) {
        int a = 0;
        for (int i = 0; i < 256; ++i) { const int v = scan[i]; scan[i] = a; a += v; }
        scan[256] = a;
        expired[l] = a;
    }
    __syncthreads();
    unsigned j = (unsigned)scan[t];
    for (int k = k0; k < k1; ++k) {
        if (!(csn[k] < thr)) continue;
        float r[RVQ_MAXD];
        rvq_residual(r, z, w.cb0, idx, (long)codebook_draw(seed, (unsigned)l, draw, j++, (unsigned)N), l, D, HW, K, L);
        cs[k] = thr;
#pragma unroll
        for (int d = 0; d < RVQ_MAXD; ++d)
            if (d < D) { cb[k * D + d] = r[d]; ea[k * D + d] = r[d] * thr; }
    }
}

// grid (ceil(K/256)): code slot j of level l <- the residual entering level l of vector pi(j)
__global__ void __launch_bounds__(256) rvq_seed_kernel(const float* z, float* cb, int l, int B, int D, int HW, int K, int L, unsigned long long seed,
                                                       unsigned draw) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= K) return;
    float r[RVQ_MAXD];
    rvq_residual(r, z, cb, nullptr, (long)codebook_draw(seed, (unsigned)l, draw, (unsigned)j, (unsigned)((long)B * HW)), l, D, HW, K, L);
#pragma unroll
    for (int d = 0; d < RVQ_MAXD; ++d)
        if (d < D) cb[((size_t)l * K + j) * D + d] = r[d];
}

static int rvq_train_shape(const char* who, int batch, int dim, int hw, int K, int L) {
    if (batch < 1 || hw < 1 || L < 1 || K < 1) return fail(FC_E_ARG, std::string(who) + ": bad argument");
    if (dim < 1 || dim > RVQ_MAXD) return fail(FC_E_SHAPE, std::string(who) + ": embedding dim must be 1..16");
    if ((size_t)L * K * dim * sizeof(float) > 64 * 1024) return fail(FC_E_SHAPE, std::string(who) + ": codebooks exceed 64 KB");
    if ((long)batch * hw > RVQ_MAX_N) return fail(FC_E_SHAPE, std::string(who) + ": more than 2^24 vectors");
    return FC_OK;
}

static int rvq_bound_launch(const float* z, const float* cb, const RvqWs& w, long n, int D, int K, int nlev, hipStream_t s) {
    const long nz = n * D;
    long g = (nz + 1023) / 1024;
    g = g < 1 ? 1 : (g > 1024 ? 1024 : g);
    hipLaunchKernelGGL(rvq_bound_kernel, dim3((unsigned)g), dim3(256), 0, s, z, nz, cb, K * D, nlev, w.maxbits);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

}  // namespace fc

extern "C" size_t fc_rvq_train_workspace_bytes(int batch, int hw, int dim, int codebook_size, int levels) {
    using namespace fc;
    if (rvq_train_shape("fc_rvq_train_workspace_bytes", batch, dim, hw, codebook_size, levels) != FC_OK) return 0;
    return ws_layout(nullptr, (long)batch * hw, dim, codebook_size, levels).bytes;
}

extern "C" int fc_codebook_draws(int64_t* out_dev, uint64_t seed, int level, int64_t draw_index, int64_t n, int64_t count, void* stream) {
    using namespace fc;
    if (!out_dev || level < 0 || count < 0 || n < 1) return fail(FC_E_ARG, "fc_codebook_draws: bad argument");
    if (draw_index < 0 || draw_index > 0xffffffffll) return fail(FC_E_ARG, "fc_codebook_draws: draw_index is a 32-bit counter word");
    if (n > RVQ_MAX_N) return fail(FC_E_SHAPE, "fc_codebook_draws: more than 2^24 vectors");
    if (!count) return FC_OK;
    hipLaunchKernelGGL(codebook_draws_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), out_dev,
                       (unsigned long long)seed, (unsigned)level, (unsigned)draw_index, (unsigned)n, (long)count);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

extern "C" int fc_rvq_seed_codes(const float* z_dev, float* codebooks_dev, int batch, int dim, int hw, int codebook_size, int levels, int level,
                                 uint64_t seed, int64_t draw_index, void* stream) {
    using namespace fc;
    FC_TRY(rvq_train_shape("fc_rvq_seed_codes", batch, dim, hw, codebook_size, levels));
    if (!z_dev || !codebooks_dev || level < 0 || level >= levels || draw_index < 0 || draw_index > 0xffffffffll)
        return fail(FC_E_ARG, "fc_rvq_seed_codes: bad argument");
    hipLaunchKernelGGL(rvq_seed_kernel, dim3((unsigned)((codebook_size + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), z_dev,
                       codebooks_dev, level, batch, dim, hw, codebook_size, levels, (unsigned long long)seed, (unsigned)draw_index);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

extern "C" int fc_rvq_kmeans(const float* z_dev, float* codebooks_dev, int batch, int dim, int hw, int codebook_size, int levels, int level, int iters,
                             float* cluster_size_out_dev, float* embed_avg_out_dev, double* objective_out_dev, void* ws_dev, size_t ws_bytes,
                             void* stream) {
    using namespace fc;
    FC_TRY(rvq_train_shape("fc_rvq_kmeans", batch, dim, hw, codebook_size, levels));
    if (!z_dev || !codebooks_dev || !ws_dev || level < 0 || level >= levels || iters < 0 || !cluster_size_out_dev != !embed_avg_out_dev)
        return fail(FC_E_ARG, "fc_rvq_kmeans: bad argument");
    const long n = (long)batch * hw;
    const int K = codebook_size, D = dim;
    const RvqWs w = ws_layout(ws_dev, n, D, K, levels);
    if (ws_bytes < w.bytes) return fail(FC_E_ARG, "fc_rvq_kmeans: workspace smaller than fc_rvq_train_workspace_bytes");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!iters) {
        if (cluster_size_out_dev) {
            FC_HIP(hipMemsetAsync(cluster_size_out_dev, 0, (size_t)K * 4, s));
            FC_HIP(hipMemsetAsync(embed_avg_out_dev, 0, (size_t)K * D * 4, s));
        }
        return FC_OK;
    }
    FC_HIP(hipMemsetAsync(ws_dev, 0, w.zero_bytes, s));
    FC_TRY(rvq_bound_launch(z_dev, codebooks_dev, w, n, D, K, level, s));     // the scale does not change with the means: once per call
    for (int it = 0; it < iters; ++it) {
        if (it) FC_HIP(hipMemsetAsync(static_cast<char*>(ws_dev) + w.acc_off, 0, w.zero_bytes - w.acc_off, s));
        hipLaunchKernelGGL(rvq_assign_kernel, dim3((unsigned)w.grid), dim3(256), (size_t)(level + 1) * K * D * sizeof(float), s, z_dev,
                           (const float*)codebooks_dev, (float*)nullptr, (int64_t*)nullptr, w, level, level, batch, D, hw, K, levels, 0);
        FC_HIP(hipGetLastError());
        const bool lastit = it == iters - 1;
        hipLaunchKernelGGL(rvq_kmeans_kernel, dim3((unsigned)((K * D + 255) / 256)), dim3(256), 0, s, codebooks_dev, w, level, K, D,
                           lastit ? cluster_size_out_dev : (float*)nullptr, lastit ? embed_avg_out_dev : (float*)nullptr,
                           objective_out_dev ? objective_out_dev + it : (double*)nullptr);
        FC_HIP(hipGetLastError());
    }
    return FC_OK;
}

extern "C" int fc_rvq_train_step(const float* z_dev, float* codebooks_dev, float* cluster_size_dev, float* embed_avg_dev, float* zq_out_dev,
                                 int64_t* indices_out_dev, float* losses_out_dev, int* expired_out_dev, int batch, int dim, int hw, int codebook_size,
                                 int levels, double decay, double commitment_weight, float threshold_ema_dead_code, uint64_t seed,
                                 int64_t draw_index, void* ws_dev, size_t ws_bytes, void* stream) {
    using namespace fc;
    FC_TRY(rvq_train_shape("fc_rvq_train_step", batch, dim, hw, codebook_size, levels));
    if (!z_dev || !codebooks_dev || !cluster_size_dev || !embed_avg_dev || !zq_out_dev || !indices_out_dev || !losses_out_dev || !expired_out_dev ||
        !ws_dev || draw_index < 0 || draw_index > 0xffffffffll || !(decay >= 0.0 && decay <= 1.0))
        return fail(FC_E_ARG, "fc_rvq_train_step: bad argument");
    const long n = (long)batch * hw;
    const int K = codebook_size, D = dim, L = levels;
    const RvqWs w = ws_layout(ws_dev, n, D, K, L);
    if (ws_bytes < w.bytes) return fail(FC_E_ARG, "fc_rvq_train_step: workspace smaller than fc_rvq_train_workspace_bytes");
    hipStream_t s = static_cast<hipStream_t>(stream);
    FC_HIP(hipMemsetAsync(ws_dev, 0, w.zero_bytes, s));
    FC_TRY(rvq_bound_launch(z_dev, codebooks_dev, w, n, D, K, L - 1, s));
    hipLaunchKernelGGL(rvq_assign_kernel, dim3((unsigned)w.grid), dim3(256), (size_t)L * K * D * sizeof(float), s, z_dev, (const float*)codebooks_dev,
                       zq_out_dev, indices_out_dev, w, 0, L - 1, batch, D, hw, K, L, 1);
    FC_HIP(hipGetLastError());
    static bool lds_set = false;                          // K floats next to 3 KB of static LDS pass 64 KB at K = 16384
    if (!lds_set) {
        FC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(rvq_ema_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
        lds_set = true;
    }
    hipLaunchKernelGGL(rvq_ema_kernel, dim3((unsigned)L), dim3(256), (size_t)K * sizeof(float), s, z_dev, codebooks_dev, cluster_size_dev,
                       embed_avg_dev, (const int64_t*)indices_out_dev, w, losses_out_dev, expired_out_dev, batch, D, hw, K, L, decay,
                       commitment_weight, threshold_ema_dead_code, (unsigned long long)seed, (unsigned)draw_index);
    FC_HIP(hipGetLastError());
    return FC_OK;
}
