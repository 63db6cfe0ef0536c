// Evaluation metrics on the device: the confusion counts of flocoder/metrics.py:362-455 (calc_note_metrics) and the per-level index
// histogram of flocoder/codebook_analysis.py:28-44 (CodebookUsageTracker.update_counts).  Both end in exact int64 counts; nothing here
// waits for the host or allocates.
//
// fc_note_confusion.  A piano roll is [B,C,H,W] fp32 with C = 3 (taken as it is) or C = 1 (g2rgb, metrics.py:319-327: red = gf >= 0.75,
// green = |gf - 0.5| < 0.25, blue = 0; keep_gray: gf > 0.5 on all three).  Per pixel and channel (0 onset, 1 sustain), in fp32 and in
// upstream's operation order (the unit is built with -ffp-contract=off and without fast-math, so a value on a boundary decides as in torch):
//     t = ((target - lo) / range) > threshold        p = ((clamp(pred, lo, hi) - lo) / range) > threshold
// lo / hi = minval / maxval: given, or the min / max of the WHOLE converted target (a first pass leaves them in the 16-byte workspace as
// order-preserving integer keys, combined with integer atomic max, plus a word that says a NaN was seen: torch's min / max return NaN then).
// range = float(maxval - minval) formed in fp64 when both are given (torch subtracts two Python numbers before the tensor sees them),
// hi - lo in fp32 otherwise.  An all-black target gives 0 / 0: every comparison is false, every pixel a true negative, as upstream.
// clamp is torch's: NaN stays NaN (and compares false), -inf -> lo, +inf -> hi.  A pixel outside `region` (region <= 0.5) is counted nowhere
// and is 0 in every image.
//
// Counting pass: the B * H*W pixels are cut into chunks of 4096, one workgroup of four waves each, so a sample may span several workgroups
// and a workgroup may cover several small samples: it walks the samples its chunk touches, and for each reduces seven small integers
// (pixels counted, tp / fp / fn of both channels; tn is the rest) in the wave by shuffles, across the waves through LDS, and adds the
// eight totals into counts[2][B][4] with 64-bit vector atomics: integer sums, so the order of arrival cannot show.  Loads and image stores
// are 16 bytes per lane when H*W is a multiple of 4 and every pointer is 16-byte aligned; any other call runs the same kernel one pixel
// per lane (a misaligned base pointer is handled, not refused).  Blue is never read here: one HBM read of red and green of both tensors.
//
// fc_index_histogram.  indices [N][L] int64 as fc_rvq_quantize writes them; counts[L][K] += the rows' indices; keys[n] = sum_l idx_l K^l.
// A row with an index outside [0, K) is counted at NO level, gets key -1 and adds one to *bad_rows: the caller reads that word when it next
// looks at the counts (the tracker raises then).  Up to FC_HIST_LDS_BINS = 8192 bins (L K <= 8192) the workgroup counts into 32-bit
// bins in LDS with LDS atomics (a workgroup sees fewer than 2^32 rows) and flushes one 64-bit global atomic per non-zero bin; above that
// every index is one 64-bit global atomic.  Latency / atomic bound: at the workload's 65,536 x 4 indices the input is 2 MB.
#include "common.h"

namespace fc {

constexpr int EM_THREADS = 256;
constexpr int EM_CHUNK = EM_THREADS * 16;          // pixels of one workgroup: a multiple of 4

struct NoteArgs {
    const float *pred, *target, *region;
    int pc, tc, B, keep_gray;
    long long n, total;                            // pixels per sample, pixels in all
    float thr, lo, hi, range;
    int derive_lo, derive_hi;
    unsigned* ws;                                  // {~key(min), key(max), NaN seen, -}
    unsigned long long* counts;                    // [2][B][4]: tp, tn, fp, fn
    float *masks, *overlay;                        // [2][4][B][n], [2][B][3][n] or null
};

// fp32 -> unsigned that sorts like the number (no NaN comes here)
__device__ __forceinline__ unsigned em_key(float x) {
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float em_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

template <int V> struct EmVec { float v[V]; };
template <int V> __device__ __forceinline__ EmVec<V> em_load(const float* p) {
    EmVec<V> r;
    if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
    } else {
        r.v[0] = p[0];
    }
    return r;
}
template <int V> __device__ __forceinline__ void em_store(float* p, const EmVec<V>& r) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else p[0] = r.v[0];
}

// g2rgb of one grey value: red and green (blue is 0, or the same again under keep_gray)
__device__ __forceinline__ void em_g2rg(float gf, int keep_gray, float& r, float& g) {
    if (keep_gray) {
        r = g = gf > 0.5f ? 1.f : 0.f;
    } else {
        r = gf >= 0.75f ? 1.f : 0.f;
        g = fabsf(gf - 0.5f) < 0.25f ? 1.f : 0.f;
    }
}

// red and green of V pixels of sample b from p on
template <int V> __device__ __forceinline__ void em_rg(const float* img, int C, long long n, long long b, long long p, int keep_gray,
                                                       EmVec<V>& r, EmVec<V>& g) {
    const float* s = img + ((size_t)b * C) * n + p;
    if (C == 3) {
        r = em_load<V>(s);
        g = em_load<V>(s + n);
        return;
    }
    const EmVec<V> gf = em_load<V>(s);
#pragma unroll
    for (int k = 0; k < V; ++k) em_g2rg(gf.v[k], keep_gray, r.v[k], g.v[k]);
}

__device__ __forceinline__ int em_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;                                                   // lane 0 holds the sum
}

// min / max (and "a NaN was seen") of the converted target: every element of a 3-channel tensor, {red, green, 0} or the binary value of a
// 1-channel one.  count = the number of floats stored
__global__ void __launch_bounds__(EM_THREADS) note_minmax_kernel(const float* t, long long count, int C, int keep_gray, int vec, unsigned* ws) {
    __shared__ float smn[EM_THREADS / 64], smx[EM_THREADS / 64];
    __shared__ int snan[EM_THREADS / 64];
    float mn = INFINITY, mx = -INFINITY;
    int nan = 0;
    auto take = [&](float x) {
        if (C == 3) {
            nan |= x != x;
            mn = fminf(mn, x);                                  // fminf / fmaxf skip a NaN operand: the flag carries it
            mx = fmaxf(mx, x);
        } else {
            float r, g;
            em_g2rg(x, keep_gray, r, g);
            mn = fminf(mn, keep_gray ? r : 0.f);
            mx = fmaxf(mx, fmaxf(r, g));
        }
    };
    const long long tid = (long long)blockIdx.x * EM_THREADS + threadIdx.x, stride = (long long)gridDim.x * EM_THREADS;
    const long long body = vec ? count & ~3ll : 0;
    for (long long e = tid * 4; e < body; e += stride * 4) {
        const float4 q = *reinterpret_cast<const float4*>(t + e);
        take(q.x); take(q.y); take(q.z); take(q.w);
    }
    for (long long e = body + tid; e < count; e += stride) take(t[e]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_down(mn, o));
        mx = fmaxf(mx, __shfl_down(mx, o));
        nan |= __shfl_down(nan, o);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { smn[wave] = mn; smx[wave] = mx; snan[wave] = nan; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < EM_THREADS / 64; ++w) { mn = fminf(mn, smn[w]); mx = fmaxf(mx, smx[w]); nan |= snan[w]; }
        atomicMax(&ws[0], ~em_key(mn));
        atomicMax(&ws[1], em_key(mx));
        if (nan) atomicOr(&ws[2], 1u);
    }
}

template <int V, bool IMG>
__global__ void __launch_bounds__(EM_THREADS) note_confusion_kernel(NoteArgs a) {
    __shared__ int red[EM_THREADS / 64][7];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n = a.n;
    const long long c0 = (long long)blockIdx.x * EM_CHUNK, c1 = c0 + EM_CHUNK < a.total ? c0 + EM_CHUNK : a.total;

    float lo = a.lo, hi = a.hi, range = a.range;
    if (a.derive_lo || a.derive_hi) {
        const bool nan = a.ws[2] != 0u;
        if (a.derive_lo) lo = nan ? NAN : em_unkey(~a.ws[0]);
        if (a.derive_hi) hi = nan ? NAN : em_unkey(a.ws[1]);
        range = hi - lo;
    }
    const float thr = a.thr;
    const size_t plane = (size_t)a.B * n;

    for (long long b = c0 / n; b * n < c1; ++b) {
        const long long s0 = (c0 > b * n ? c0 : b * n) - b * n, s1 = (c1 < (b + 1) * n ? c1 : (b + 1) * n) - b * n;
        int cnt[7] = {0, 0, 0, 0, 0, 0, 0};
        for (long long p = s0 + (long long)tid * V; p < s1; p += EM_THREADS * V) {      // V = 4: n, and with it s0 and s1, are multiples of 4
            EmVec<V> pv[2], tv[2], rg;
            em_rg<V>(a.pred, a.pc, n, b, p, a.keep_gray, pv[0], pv[1]);
            em_rg<V>(a.target, a.tc, n, b, p, a.keep_gray, tv[0], tv[1]);
            if (a.region) rg = em_load<V>(a.region + b * n + p);
            EmVec<V> im[2][6];                                                          // tp, tn, fp, fn, target bit, pred bit
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const bool in = a.region ? rg.v[k] > 0.5f : true;
                cnt[0] += in;
#pragma unroll
                for (int ch = 0; ch < 2; ++ch) {
                    const float x = pv[ch].v[k];
                    const float xc = x != x ? x : fminf(fmaxf(x, lo), hi);
                    const bool tb = in && ((tv[ch].v[k] - lo) / range) > thr;
                    const bool pb = in && ((xc - lo) / range) > thr;
                    cnt[1 + 3 * ch] += tb && pb;
                    cnt[2 + 3 * ch] += pb && !tb;
                    cnt[3 + 3 * ch] += tb && !pb;
                    if (IMG) {
                        im[ch][0].v[k] = tb && pb ? 1.f : 0.f;
                        im[ch][1].v[k] = in && !tb && !pb ? 1.f : 0.f;
                        im[ch][2].v[k] = pb && !tb ? 1.f : 0.f;
                        im[ch][3].v[k] = tb && !pb ? 1.f : 0.f;
                        im[ch][4].v[k] = tb ? 1.f : 0.f;
                        im[ch][5].v[k] = pb ? 1.f : 0.f;
                    }
                }
            }
            if (IMG) {
                EmVec<V> zero;
#pragma unroll
                for (int k = 0; k < V; ++k) zero.v[k] = 0.f;
#pragma unroll
                for (int ch = 0; ch < 2; ++ch) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) em_store<V>(a.masks + (size_t)(ch * 4 + q) * plane + b * n + p, im[ch][q]);
                    float* ov = a.overlay + ((size_t)ch * a.B + b) * 3 * n + p;
                    em_store<V>(ov, im[ch][4]);
                    em_store<V>(ov + n, im[ch][5]);
                    em_store<V>(ov + 2 * n, zero);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            const int v = em_wave_sum(cnt[i]);
            if (lane == 0) red[wave][i] = v;
        }
        __syncthreads();
        if (tid < 8) {
            const int ch = tid >> 2, q = tid & 3;
            int m = 0, tp = 0, fp = 0, fn = 0;
            for (int w = 0; w < EM_THREADS / 64; ++w) {
                m += red[w][0]; tp += red[w][1 + 3 * ch]; fp += red[w][2 + 3 * ch]; fn += red[w][3 + 3 * ch];
            }
            const int v = q == 0 ? tp : q == 1 ? m - tp - fp - fn : q == 2 ? fp : fn;
            if (v) atomicAdd(&a.counts[((size_t)ch * a.B + b) * 4 + q], (unsigned long long)v);
        }
        __syncthreads();
    }
}

constexpr int HG_THREADS = 256;
constexpr int HG_ROWS_PER_BLOCK = 1024, HG_MAX_BLOCKS = 1024;

template <bool LDS>
__global__ void __launch_bounds__(HG_THREADS) index_histogram_kernel(const long long* idx, long long N, int L, int K, unsigned long long* counts,
                                                                     long long* keys, unsigned long long* bad) {
    extern __shared__ unsigned hg_bins[];                       // [L][K] when LDS
    const int tid = threadIdx.x;
    if (LDS) {
        for (int i = tid; i < L * K; i += HG_THREADS) hg_bins[i] = 0u;
        __syncthreads();
    }
    for (long long i = (long long)blockIdx.x * HG_THREADS + tid; i < N; i += (long long)gridDim.x * HG_THREADS) {
        const long long* row = idx + i * L;
        bool ok = true;
        for (int l = 0; l < L; ++l) ok = ok && row[l] >= 0 && row[l] < K;
        if (!ok) {                                              // counted nowhere, reported
            atomicAdd(bad, 1ull);
            if (keys) keys[i] = -1;
            continue;
        }
        unsigned long long key = 0ull, mult = 1ull;
        for (int l = 0; l < L; ++l) {
            const unsigned long long v = (unsigned long long)row[l];
            if (LDS) atomicAdd(&hg_bins[l * K + (int)v], 1u);
            else atomicAdd(&counts[(size_t)l * K + v], 1ull);
            key += v * mult;
            mult *= (unsigned long long)K;
        }
        if (keys) keys[i] = (long long)key;
    }
    if (LDS) {
        __syncthreads();
        for (int i = tid; i < L * K; i += HG_THREADS) {
            const unsigned c = hg_bins[i];
            if (c) atomicAdd(&counts[i], (unsigned long long)c);
        }
    }
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace fc

using namespace fc;

extern "C" {

int fc_note_confusion(const float* pred_dev, int pred_channels, const float* target_dev, int target_channels, const float* region_dev, int batch,
                      int height, int width, float threshold, double minval, int derive_min, double maxval, int derive_max, int keep_gray,
                      void* ws_dev, int64_t* counts_out_dev, float* masks_out_dev, float* overlay_out_dev, void* stream) {
    if (!pred_dev || !target_dev || !ws_dev || !counts_out_dev) return fail(FC_E_ARG, "fc_note_confusion: null argument");
    if ((masks_out_dev == nullptr) != (overlay_out_dev == nullptr))
        return fail(FC_E_ARG, "fc_note_confusion: the mask images and the overlays come together or not at all");
    if ((pred_channels != 1 && pred_channels != 3) || (target_channels != 1 && target_channels != 3))
        return fail(FC_E_SHAPE, "fc_note_confusion: a piano roll has 1 or 3 channels");
    if (batch < 1 || height < 1 || width < 1) return fail(FC_E_SHAPE, "fc_note_confusion: batch, height and width must be positive");
    const long long n = (long long)height * width, total = n * batch;
    if (total > (1ll << 40)) return fail(FC_E_SHAPE, "fc_note_confusion: more than 2^40 pixels");
    if ((reinterpret_cast<uintptr_t>(pred_dev) | reinterpret_cast<uintptr_t>(target_dev) | reinterpret_cast<uintptr_t>(region_dev) |
         reinterpret_cast<uintptr_t>(masks_out_dev) | reinterpret_cast<uintptr_t>(overlay_out_dev) | reinterpret_cast<uintptr_t>(ws_dev)) & 3)
        return fail(FC_E_ARG, "fc_note_confusion: a float pointer that is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(counts_out_dev) & 7) return fail(FC_E_ARG, "fc_note_confusion: counts must be 8-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    FC_HIP(hipMemsetAsync(counts_out_dev, 0, sizeof(int64_t) * 8 * (size_t)batch, s));
    NoteArgs a = {};
    a.pred = pred_dev; a.target = target_dev; a.region = region_dev;
    a.pc = pred_channels; a.tc = target_channels; a.B = batch; a.keep_gray = keep_gray != 0;
    a.n = n; a.total = total;
    a.thr = threshold; a.lo = (float)minval; a.hi = (float)maxval; a.range = (float)(maxval - minval);
    a.derive_lo = derive_min != 0; a.derive_hi = derive_max != 0;
    a.ws = static_cast<unsigned*>(ws_dev);
    a.counts = reinterpret_cast<unsigned long long*>(counts_out_dev);
    a.masks = masks_out_dev; a.overlay = overlay_out_dev;
    if (a.derive_lo || a.derive_hi) {
        FC_HIP(hipMemsetAsync(ws_dev, 0, 16, s));
        const long long count = total * target_channels;
        const long long want = (count + EM_CHUNK - 1) / EM_CHUNK;
        const int grid = (int)(want < 1024 ? want : 1024);
        hipLaunchKernelGGL(note_minmax_kernel, dim3(grid), dim3(EM_THREADS), 0, s, target_dev, count, target_channels, a.keep_gray,
                           aligned16(target_dev) ? 1 : 0, a.ws);
        FC_HIP(hipGetLastError());
    }
    const bool vec = (n & 3) == 0 && aligned16(pred_dev) && aligned16(target_dev) && aligned16(region_dev) && aligned16(masks_out_dev) &&
                     aligned16(overlay_out_dev);
    const long long grid = (total + EM_CHUNK - 1) / EM_CHUNK;
    const bool img = masks_out_dev != nullptr;
    auto kernel = vec ? (img ? note_confusion_kernel<4, true> : note_confusion_kernel<4, false>)
                      : (img ? note_confusion_kernel<1, true> : note_confusion_kernel<1, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(EM_THREADS), 0, s, a);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

int fc_index_histogram(const int64_t* indices_dev, int64_t n, int levels, int codebook_size, int64_t* counts_inout_dev, int64_t* keys_out_dev,
                       int64_t* bad_rows_inout_dev, void* stream) {
    if (!indices_dev || !counts_inout_dev || !bad_rows_inout_dev) return fail(FC_E_ARG, "fc_index_histogram: null argument");
    if (n < 0 || levels < 1 || codebook_size < 1) return fail(FC_E_SHAPE, "fc_index_histogram: n >= 0, levels >= 1 and codebook_size >= 1");
    if ((long long)levels * codebook_size > (1ll << 30)) return fail(FC_E_SHAPE, "fc_index_histogram: more than 2^30 bins");
    if ((reinterpret_cast<uintptr_t>(indices_dev) | reinterpret_cast<uintptr_t>(counts_inout_dev) | reinterpret_cast<uintptr_t>(keys_out_dev) |
         reinterpret_cast<uintptr_t>(bad_rows_inout_dev)) & 7)
        return fail(FC_E_ARG, "fc_index_histogram: an int64 pointer that is not 8-byte aligned");
    if (keys_out_dev) {
        long long p = 1;                                        // K^L must be an int64 for the keys to tell combinations apart
        for (int l = 0; l < levels; ++l) {
            if (p > INT64_MAX / codebook_size) return fail(FC_E_SHAPE, "fc_index_histogram: codebook_size^levels overflows int64, no keys");
            p *= codebook_size;
        }
    }
    if (n == 0) return FC_OK;
    const long long want = (n + HG_ROWS_PER_BLOCK - 1) / HG_ROWS_PER_BLOCK;
    const int grid = (int)(want < HG_MAX_BLOCKS ? want : HG_MAX_BLOCKS);
    const int bins = levels * codebook_size;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long* idx = reinterpret_cast<const long long*>(indices_dev);
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(counts_inout_dev);
    long long* keys = reinterpret_cast<long long*>(keys_out_dev);
    unsigned long long* bad = reinterpret_cast<unsigned long long*>(bad_rows_inout_dev);
    if (bins <= FC_HIST_LDS_BINS)
        hipLaunchKernelGGL(index_histogram_kernel<true>, dim3(grid), dim3(HG_THREADS), sizeof(unsigned) * bins, s, idx, (long long)n, levels,
                           codebook_size, counts, keys, bad);
    else
        hipLaunchKernelGGL(index_histogram_kernel<false>, dim3(grid), dim3(HG_THREADS), 0, s, idx, (long long)n, levels, codebook_size, counts,
                           keys, bad);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

}  // extern "C"
