// Inpainting masks on the device: a counter-based restatement of upstream's generate_mask (flocoder/inpainting.py:277-351).  A mask is a
// function of (seed, sample id, H, W, type probabilities | forced type) and of nothing else; flocoder_amd/noise.py (mask_field) is the host
// form and the two agree in every bit, because every draw and the whole brush walk are integer arithmetic.
//
// Philox key = seed + FC_MASK_KEY_OFFSET (mod 2^64); counter = (j, region, sample id lo, sample id hi):
//   region 0, j = 0          word 0: the type, against the 32-bit thresholds floor(cum_k 2^32) of the cumulative probabilities;
//                            word 1: the number of brush strokes 2 + mulhi(w, 4); word 2: the number of rectangles 2 + mulhi(w, 9)
//   region 1, j              'noise': pixels 4j .. 4j+3 of the flattened image, set where (w >> 9) >= 5872026 (the uniform exceeds 0.7)
//   region 2, j = rectangle  words 0..3: w, h, x, y of generate_rectangles, in that order
//   region 3 + s, j = 0      stroke s: words 0..3: bs, start x, start y, length;  j = 1: word 0: the start direction
//   region 3 + s, j = 2 + t  step t: kick = sum_k mulhi(w_k, 723) - 1444; radius offset = ((w_3 & 0xffff) * bs) >> 16
// randint(lo, hi) = lo + mulhi(w, hi - lo).  x is a column in [0, W), y a row in [0, H) everywhere (noise.py says how that differs from
// upstream at non-square sizes).
//
// The walk in integers: the direction is a binary angle in units of 2 pi / 65536 (only its value mod 2^16 matters), the kick a sum of four
// uniforms on [0, 723) minus 1444 (std 417 units = 0.040 rad), the step MASK_TRIG[d >> 4] (cosine) and MASK_TRIG[(d >> 4) - 1024] (sine) of
// the committed table mask_trig.h -- 0.7 px in Q16 -- and the pixel is position >> 16.  No cosf / logf: theirs and libm's differ in the
// last bits, and a float walk would put some disc centres on different pixels on the two sides.
//
// Shape: one workgroup of four waves per sample.  The stroke stops at the first step that leaves the image, so direction, position and
// that step are prefix sums of independent draws: a wave owns a stroke and scans 64 steps at a time (shuffles for the sums, a ballot for
// the exit), writing the surviving stamps (centre, radius) to LDS: at most 5 x 300.  Rasterisation paints a 1-bit image in LDS with
// atomicOr on LDS words: a work item is (stamp, row offset) -> the disc's span on that row (half widths of every radius up to 20 from a
// small integer table built in LDS) -> at most three 32-bit words.  The bit image holds 8192 words (32 KB): 128 x 128 is 512 of them, and
// an image with more than 2^18 pixels is painted in bands of rows, every band looking at all stamps.  A band is then written as fp32,
// 16 bytes per lane where the row length allows.  Every loop is bounded by a constant or by H W; nothing is allocated, nothing but the
// output is written to memory, and there is no atomic on it.
#include "common.h"
#include "mask_trig.h"
#include "philox.h"

namespace fc {

constexpr int MK_THREADS = 256;
constexpr int MK_STROKES = 5, MK_STEPS = 300, MK_RECTS = 10, MK_RADIUS = 20;
constexpr int MK_IMG_WORDS = 8192;
constexpr int MK_CHOICES = 16;
constexpr unsigned MK_NOISE_THRESHOLD = 5872026u;

struct MaskTypeTable {
    unsigned long long thr[MK_CHOICES];   // floor(cum_k 2^32); the last live one is 2^32
    int code[MK_CHOICES];
    int n, forced;                        // forced >= 0: that type for every sample
};

__device__ __forceinline__ int mk_mulhi(unsigned w, int n) { return (int)__umulhi(w, (unsigned)n); }

__device__ __forceinline__ int wave_scan(int v, int lane) {   // inclusive prefix sum over the 64 lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

// o[p] = f(p) for p in [0, n): float4 stores when vec (n a multiple of 4 and o 16-byte aligned)
template <typename F>
__device__ __forceinline__ void mk_write(float* o, int n, bool vec, F f) {
    if (vec) {
        for (int p = threadIdx.x * 4; p < n; p += MK_THREADS * 4)
            *reinterpret_cast<float4*>(o + p) = make_float4(f(p), f(p + 1), f(p + 2), f(p + 3));
    } else {
        for (int p = threadIdx.x; p < n; p += MK_THREADS) o[p] = f(p);
    }
}

__global__ void __launch_bounds__(MK_THREADS) inpaint_masks_kernel(float* out, int* types_out, unsigned long long key, const long long* sids,
                                                                   int H, int W, MaskTypeTable tt) {
    __shared__ unsigned img[MK_IMG_WORDS];
    __shared__ int stamp_xy[MK_STROKES * MK_STEPS];             // column | row << 16
    __shared__ unsigned char stamp_r[MK_STROKES * MK_STEPS];
    __shared__ int stroke_cnt[MK_STROKES];
    __shared__ signed char half_w[(MK_RADIUS + 1) * (MK_RADIUS + 1)];
    __shared__ int4 rect[MK_RECTS];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long sid = sids ? (unsigned long long)sids[b] : (unsigned long long)b;
    const unsigned s0 = (unsigned)sid, s1 = (unsigned)(sid >> 32), k0 = (unsigned)key, k1 = (unsigned)(key >> 32);
    const int n = H * W;
    float* o = out + (size_t)b * n;
    const bool vec = (n & 3) == 0 && (reinterpret_cast<uintptr_t>(o) & 15) == 0;

    unsigned hd[4];
    philox4x32_10(0u, 0u, s0, s1, k0, k1, hd);
    int type = tt.forced;
    if (type < 0) {
        int k = 0;                                              // the thresholds do not decrease: the number of them at or below the word
        for (int i = 0; i < MK_CHOICES - 1; ++i)
            if (i < tt.n - 1 && (unsigned long long)hd[0] >= tt.thr[i]) k = i + 1;
        type = tt.code[k];
    }
    if (tid == 0) types_out[b] = type;                          // the type is the same in every thread: the branches below are uniform

    if (type == FC_MASK_TOTAL || type == FC_MASK_NOTHING) {
        const float v = type == FC_MASK_TOTAL ? 1.f : 0.f;
        mk_write(o, n, vec, [&](int) { return v; });
        return;
    }
    if (type == FC_MASK_NOISE) {
        for (int j = tid; j < (n + 3) / 4; j += MK_THREADS) {
            unsigned r[4];
            philox4x32_10((unsigned)j, 1u, s0, s1, k0, k1, r);
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = (r[k] >> 9) >= MK_NOISE_THRESHOLD ? 1.f : 0.f;
            if (vec) {
                *reinterpret_cast<float4*>(o + 4 * j) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (4 * j + k < n) o[4 * j + k] = v[k];
            }
        }
        return;
    }
    if (type == FC_MASK_RECTANGLES) {
        const int n_rect = 2 + mk_mulhi(hd[2], 9);
        if (tid < MK_RECTS) {
            unsigned r[4];
            philox4x32_10((unsigned)tid, 2u, s0, s1, k0, k1, r);
            const int rw = 3 + mk_mulhi(r[0], (W * 4) / 5 - 3), rh = 3 + mk_mulhi(r[1], (H * 3) / 10 - 3);
            const int rx = mk_mulhi(r[2], W - rw), ry = mk_mulhi(r[3], H - rh);
            rect[tid] = make_int4(rx, ry, rx + rw, ry + rh);
        }
        __syncthreads();
        mk_write(o, n, vec, [&](int p) {
            const int y = p / W, x = p - y * W;
            bool hit = false;
            for (int k = 0; k < MK_RECTS; ++k) {
                const int4 q = rect[k];
                hit |= k < n_rect && x >= q.x && x < q.z && y >= q.y && y < q.w;
            }
            return hit ? 1.f : 0.f;
        });
        return;
    }

    // ---- brush ----
    const int n_strokes = 2 + mk_mulhi(hd[1], 4);
    if (tid < MK_STROKES) stroke_cnt[tid] = 0;
    for (int i = tid; i < (MK_RADIUS + 1) * (MK_RADIUS + 1); i += MK_THREADS) {
        const int cb = i / (MK_RADIUS + 1), dy = i % (MK_RADIUS + 1);
        int h = -1;
        for (int k = 0; k <= MK_RADIUS; ++k)
            if (k * k + dy * dy <= cb * cb) h = k;
        half_w[i] = (signed char)h;
    }
    __syncthreads();
    for (int s = wave; s < n_strokes; s += MK_THREADS / 64) {
        unsigned r[4];
        philox4x32_10(0u, 3u + s, s0, s1, k0, k1, r);
        const int bs = 3 + mk_mulhi(r[0], 12), x0 = mk_mulhi(r[1], W), y0 = H / 3 + mk_mulhi(r[2], 2 * H / 3 - H / 3);
        const int len = 100 + mk_mulhi(r[3], 200);
        philox4x32_10(1u, 3u + s, s0, s1, k0, k1, r);
        int d = mk_mulhi(r[0], 2 * 3277 + 1) - 3277 + (2 * x0 > W ? 32768 : 0);
        int X = x0 << 16, Y = y0 << 16, cnt = 0;
        bool stop = false;
        for (int c = 0; c < (MK_STEPS + 63) / 64; ++c) {
            if (stop) continue;                                 // wave-uniform
            const int t = c * 64 + lane;
            const bool active = t < len;
            int kick = 0, cb = 1;
            if (active) {
                philox4x32_10(2u + t, 3u + s, s0, s1, k0, k1, r);
                kick = mk_mulhi(r[0], 723) + mk_mulhi(r[1], 723) + mk_mulhi(r[2], 723) + mk_mulhi(r[3], 723) - 1444;
                cb = bs - ((bs + 1) >> 1) + (int)(((r[3] & 0xffffu) * (unsigned)bs) >> 16);     // bs + randint(-bs//2, bs//2), floor division
                cb = cb < 1 ? 1 : cb;
            }
            const int ks = wave_scan(kick, lane);
            const int a = ((d + ks) & 0xffff) >> (16 - FC_MASK_TRIG_BITS);
            const int cx = active ? MASK_TRIG[a] : 0;
            const int sy = active ? MASK_TRIG[(a - (1 << (FC_MASK_TRIG_BITS - 2))) & ((1 << FC_MASK_TRIG_BITS) - 1)] : 0;
            const int cxs = wave_scan(cx, lane), sys = wave_scan(sy, lane);
            const int px = X + cxs, py = Y + sys;
            const bool gone = active && (px < 0 || px >= (W << 16) || py < 0 || py >= (H << 16));
            const unsigned long long m = __ballot(gone);
            const int first = m ? __ffsll((long long)m) - 1 : 64;
            if (active && lane < first) {
                stamp_xy[s * MK_STEPS + t] = (px >> 16) | ((py >> 16) << 16);
                stamp_r[s * MK_STEPS + t] = (unsigned char)cb;
            }
            const int live = len - c * 64 < 64 ? len - c * 64 : 64;          // active lanes of this chunk (may be <= 0)
            cnt += first < live ? first : (live > 0 ? live : 0);
            stop = m != 0ull || live < 64;
            d += __shfl(ks, 63); X += __shfl(cxs, 63); Y += __shfl(sys, 63);
        }
        if (lane == 0) stroke_cnt[s] = cnt;
    }
    __syncthreads();

    const int wpr = (W + 31) >> 5;                              // words per row: at most 32
    const int band = MK_IMG_WORDS / wpr < H ? MK_IMG_WORDS / wpr : H;
    for (int yb = 0; yb < H; yb += band) {
        const int rows = H - yb < band ? H - yb : band;
        for (int i = tid; i < rows * wpr; i += MK_THREADS) img[i] = 0u;
        __syncthreads();
        for (int s = 0; s < MK_STROKES; ++s) {
            const int items = stroke_cnt[s] * (2 * MK_RADIUS + 1);
            for (int i = tid; i < items; i += MK_THREADS) {
                const int st = s * MK_STEPS + i / (2 * MK_RADIUS + 1), dy = i % (2 * MK_RADIUS + 1) - MK_RADIUS;
                const int cb = stamp_r[st], ady = dy < 0 ? -dy : dy;
                const int xy = stamp_xy[st], row = (xy >> 16) + dy - yb;
                if (ady > cb || row < 0 || row >= rows) continue;
                const int hw = half_w[cb * (MK_RADIUS + 1) + ady], xi = xy & 0xffff;
                const int xl = xi - hw < 0 ? 0 : xi - hw, xr = xi + hw > W - 1 ? W - 1 : xi + hw;
                for (int wd = xl >> 5; wd <= (xr >> 5); ++wd) {                                  // a span of <= 41 pixels: <= 3 words
                    const int lo = xl > wd * 32 ? xl - wd * 32 : 0, hi = xr < wd * 32 + 31 ? xr - wd * 32 : 31;
                    const unsigned bits = (0xffffffffu >> (31 - (hi - lo))) << lo;
                    atomicOr(&img[row * wpr + wd], bits);
                }
            }
        }
        __syncthreads();
        float* ob = o + (size_t)yb * W;
        mk_write(ob, rows * W, vec && (W & 3) == 0, [&](int p) {
            const int y = p / W, x = p - y * W;
            return (float)((img[y * wpr + (x >> 5)] >> (x & 31)) & 1u);
        });
        __syncthreads();
    }
}

}  // namespace fc

using namespace fc;

extern "C" {

int fc_inpaint_masks(float* masks_out_dev, int* types_out_dev, uint64_t seed, const int64_t* sample_ids_dev, int batch, int height, int width,
                     const int* choice_types_host, const double* probs_host, int n_choices, int forced_type, void* stream) {
    if (!masks_out_dev || !types_out_dev) return fail(FC_E_ARG, "fc_inpaint_masks: null argument");
    if (height < FC_MASK_MIN_SIZE || height > FC_MASK_MAX_SIZE || width < FC_MASK_MIN_SIZE || width > FC_MASK_MAX_SIZE)
        return fail(FC_E_SHAPE, "fc_inpaint_masks: height and width must lie in [16, 1024]");
    if (batch < 1) return fail(FC_E_SHAPE, "fc_inpaint_masks: batch must be positive");
    MaskTypeTable tt = {};
    tt.forced = -1;
    tt.n = 1;
    if (forced_type >= 0) {
        if (forced_type > FC_MASK_NOTHING) return fail(FC_E_ARG, "fc_inpaint_masks: unknown forced type");
        tt.forced = forced_type;
    } else {
        if (!choice_types_host || !probs_host || n_choices < 1 || n_choices > MK_CHOICES)
            return fail(FC_E_ARG, "fc_inpaint_masks: 1 to 16 choices with their probabilities, or a forced type");
        double cum = 0.0;
        for (int k = 0; k < n_choices; ++k) {
            if (choice_types_host[k] < 0 || choice_types_host[k] > FC_MASK_NOTHING) return fail(FC_E_ARG, "fc_inpaint_masks: unknown type among the choices");
            if (!(probs_host[k] >= 0.0 && probs_host[k] <= 1.0)) return fail(FC_E_ARG, "fc_inpaint_masks: a probability outside [0, 1]");
            cum += probs_host[k];
            const double t = cum * 4294967296.0;                // exact; the floor below is too
            tt.thr[k] = t >= 4294967296.0 ? 4294967296ull : (unsigned long long)t;
            tt.code[k] = choice_types_host[k];
        }
        if (!(cum > 1.0 - 1e-8 && cum < 1.0 + 1e-8)) return fail(FC_E_ARG, "fc_inpaint_masks: the probabilities must sum to 1");
        tt.thr[n_choices - 1] = 4294967296ull;
        tt.n = n_choices;
    }
    const unsigned long long key = seed + FC_MASK_KEY_OFFSET;
    hipLaunchKernelGGL(inpaint_masks_kernel, dim3(batch), dim3(MK_THREADS), 0, static_cast<hipStream_t>(stream), masks_out_dev, types_out_dev, key,
                       reinterpret_cast<const long long*>(sample_ids_dev), height, width, tt);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

}  // extern "C"
