// Piano-roll images <-> note lists on the device: flocoder/pianoroll.py's img2midi_multi (regroup_lines, filter_redgreen, img2midi,
// piano_roll_to_pretty_midi) and the painting of get_piano_rolls + piano_roll_to_img (onset style 'start'), as DESIGN.md section 4
// "Piano rolls and MIDI" and flocoder_amd/pianoroll.py (the NumPy definition) state them.  Integer arithmetic only: the same bits run to run.
//
// A roll is 128 pitches x T columns (T <= FC_ROLL_MAX_COLUMNS).  Column t of image row y (pitch 127 - y) is read where the layout puts it:
//   strips (sq = 0): strip s = t / W, pixel (128 s + y, t % W);
//   squares (sq = W / 256 squares per image row: 1 for a 256 x 256 image, 8 for the 2048 x 2048 grid): square q = t / 512 at
//   (256 (q / sq), 256 (q % sq)), inside it (y, u) for u = t % 512 < 256 and (128 + y, 511 - u) behind.
//
// fc_pianoroll_scan, four launches (five for float images):
//   roll_minmax   float images only: per-image min / max as order-preserving integer keys (integer atomic max: order cannot show).
//   roll_filter   a wave per (roll, row, chunk of 8 words of 64 columns): lanes classify their pixel (R / G / Wh, thresh 20, strict),
//                 ballots give the word's R and G masks, and the onset flag of filter_redgreen runs along the word as ONE 64-bit add:
//                 the kept greens are the G runs that begin right behind an R (or behind the carried flag at bit 0), and adding those seed
//                 bits to the run mask ripples through exactly such a run.  A column that starts a row of the regrouped image (period W,
//                 512 or 2048) is cut out of the run mask, so nothing crosses it.  The flag entering a chunk is found by looking back for
//                 the last pixel that is not green (or starts a row): it is set iff that pixel is red.  Writes plane[roll][pitch][t] =
//                 velocity | (R class) << 7, rows 0 / 127 zero, separators in.
//   roll_masks    a wave per (roll, pitch, word): ballots of "a note starts here" and "a note's last column".
//   roll_prefix   a workgroup per roll: last-column bits per word over the 128 pitches, exclusive prefix over the words, the roll's count.
// fc_pianoroll_emit, one launch: a wave per (roll, word), lane = column: the lane counts its column's ends over the pitches, a shuffle
//   scan gives the column's first slot, and the note ending at (t, p) goes to slot base[word] + columns before + pitches below -- ascending
//   (end, pitch), upstream's order, decided by counting alone.  Its start is the highest start bit at or below t (a scan back over words).
// Every loop is bounded by T / 64 words or by 128 pitches.
//
// fc_pianoroll_render: a workgroup per (roll, pitch) walks the roll's note list; an entry of that pitch writes (index + 1) << 8 | value
// into the window's columns in LDS with an integer atomic max -- [start, end) its velocity, column start - 1 zero -- so a pixel ends with
// the LAST list entry that touches it, whatever order the lanes run in.  One extra column in front decides the onset of the window's first.
#include "common.h"

namespace fc {

constexpr int RL_THREADS = 256;
constexpr int RL_CHUNK = 8;                     // words of 64 columns a wave of roll_filter walks
constexpr int RL_THRESH = 20;                   // filter_redgreen's thresh

struct RollArgs {
    const void* img;                            // uint8 or float [B][3][H][W]
    int B, H, W, T, NW;                         // T columns, NW = ceil(T / 64) words
    int sq;                                     // squares per image row; 0: strips
    int period;                                 // the onset flag restarts at columns that are multiples of it
    int require, sep, split;
    const unsigned* mm;                         // float images: [B][2] keys {~key(min), key(max)}
    unsigned char* plane;                       // [B][128][T]
    unsigned long long *starts, *lasts;         // [B][128][NW]
    int* base;                                  // [B][NW]
    long long* counts;                          // [B]
};

__device__ __forceinline__ unsigned rl_key(float x) {
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float rl_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// metrics.to_uint8 of one value: ((x - min) / max(max - min, 1e-5)) * 255, clamped, truncated; fp32, IEEE division.  NaN reads as 0
__device__ __forceinline__ int rl_byte(float x, float mn, float d) {
    const float y = ((x - mn) / d) * 255.f;
    return (int)fminf(fmaxf(y, 0.f), 255.f);
}

__global__ void __launch_bounds__(RL_THREADS) roll_minmax_kernel(const float* img, long long per, unsigned* mm) {
    __shared__ float smn[RL_THREADS / 64], smx[RL_THREADS / 64];
    const float* p = img + (size_t)blockIdx.y * per;
    float mn = INFINITY, mx = -INFINITY;
    for (long long i = (long long)blockIdx.x * RL_THREADS + threadIdx.x; i < per; i += (long long)gridDim.x * RL_THREADS) {
        const float x = p[i];
        mn = fminf(mn, x);                      // a NaN operand is skipped
        mx = fmaxf(mx, x);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_down(mn, o));
        mx = fmaxf(mx, __shfl_down(mx, o));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { smn[wave] = mn; smx[wave] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < RL_THREADS / 64; ++w) { mn = fminf(mn, smn[w]); mx = fmaxf(mx, smx[w]); }
        atomicMax(&mm[2 * blockIdx.y], ~rl_key(mn));
        atomicMax(&mm[2 * blockIdx.y + 1], rl_key(mx));
    }
}

// the bytes of column t of image row y of roll b (t < T)
template <bool FLT>
__device__ __forceinline__ void rl_pixel(const RollArgs& a, int b, int y, int t, float mn, float d, int& r, int& g, int& bl) {
    int row, col;
    if (a.sq == 0) {
        row = 128 * (t / a.W) + y;
        col = t % a.W;
    } else {
        const int q = t >> 9, u = t & 511;
        row = 256 * (q / a.sq) + (u < 256 ? y : 128 + y);
        col = 256 * (q % a.sq) + (u < 256 ? u : 511 - u);
    }
    const size_t n = (size_t)a.H * a.W, at = (size_t)b * 3 * n + (size_t)row * a.W + col;
    if (FLT) {
        const float* p = static_cast<const float*>(a.img) + at;
        r = rl_byte(p[0], mn, d); g = rl_byte(p[n], mn, d); bl = rl_byte(p[2 * n], mn, d);
    } else {
        const unsigned char* p = static_cast<const unsigned char*>(a.img) + at;
        r = p[0]; g = p[n]; bl = p[2 * n];
    }
}

template <bool FLT>
__global__ void __launch_bounds__(RL_THREADS) roll_filter_kernel(RollArgs a) {
    const int lane = threadIdx.x & 63;
    const int nch = (a.NW + RL_CHUNK - 1) / RL_CHUNK;
    const long long item = (long long)blockIdx.x * (RL_THREADS / 64) + (threadIdx.x >> 6);
    if (item >= (long long)a.B * 128 * nch) return;                      // the whole wave leaves
    const int ch = (int)(item % nch), y = (int)((item / nch) % 128), b = (int)(item / ((long long)nch * 128));
    const int w0 = ch * RL_CHUNK, w1 = w0 + RL_CHUNK < a.NW ? w0 + RL_CHUNK : a.NW;
    float mn = 0.f, d = 1.f;
    if (FLT) {
        mn = rl_unkey(~a.mm[2 * b]);
        d = fmaxf(rl_unkey(a.mm[2 * b + 1]) - mn, 1e-5f);
    }
    unsigned long long cin = 0ull;
    if (a.require && w0 > 0 && (w0 * 64) % a.period != 0) {
        for (int w = w0 - 1; w >= 0; --w) {                              // every column of these words is below T
            const int t = w * 64 + lane;
            int r, g, bl;
            rl_pixel<FLT>(a, b, y, t, mn, d, r, g, bl);
            const unsigned long long R = __ballot(r > RL_THRESH && g < RL_THRESH && bl < RL_THRESH);
            const unsigned long long G = __ballot(r < RL_THRESH && g > RL_THRESH && bl < RL_THRESH);
            const unsigned long long stop = ~G | __ballot(t % a.period == 0);
            if (stop) {
                cin = (R >> (63 - __clzll((long long)stop))) & 1ull;
                break;
            }
        }
    }
    const int pitch = 127 - y;
    unsigned char* out = a.plane + ((size_t)b * 128 + pitch) * a.T;
    for (int w = w0; w < w1; ++w) {
        const int t = w * 64 + lane;
        const bool valid = t < a.T;
        int r = 0, g = 0, bl = 0;
        if (valid) rl_pixel<FLT>(a, b, y, t, mn, d, r, g, bl);
        const bool isR = r > RL_THRESH && g < RL_THRESH && bl < RL_THRESH;
        const bool isG = r < RL_THRESH && g > RL_THRESH && bl < RL_THRESH;
        const bool isW = r > RL_THRESH && g > RL_THRESH && bl > RL_THRESH;
        int val;
        if (a.require) {
            const unsigned long long R = __ballot(isR), G = __ballot(isG);
            const unsigned long long M = G & ~__ballot(valid && t % a.period == 0);
            const unsigned long long seeds = ((R << 1) | cin) & M;
            const unsigned long long kept = ((M + seeds) ^ M) & M;
            cin = (R | kept) >> 63;
            val = isR ? r : ((kept >> lane) & 1ull) ? g : 0;
        } else {
            val = isR ? r : (isG || isW) ? g : 0;
        }
        int v = val >> 1, flag = isR ? 0x80 : 0;
        if (y == 0 || y == 127) { v = 0; flag = 0; }
        if (a.sep > 0 && t > 0 && t % a.sep == 0 && pitch >= 35 && pitch <= 92) v = 30;
        if (valid) out[t] = (unsigned char)(v | flag);
    }
}

__global__ void __launch_bounds__(RL_THREADS) roll_masks_kernel(RollArgs a) {
    const int lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * (RL_THREADS / 64) + (threadIdx.x >> 6);     // (b * 128 + pitch) * NW + w
    if (item >= (long long)a.B * 128 * a.NW) return;
    const int w = (int)(item % a.NW);
    const unsigned char* row = a.plane + (size_t)(item / a.NW) * a.T;
    const int t = w * 64 + lane;
    const bool valid = t < a.T;
    const int cur = valid ? row[t] : 0, prev = valid && t > 0 ? row[t - 1] : 0, next = t + 1 < a.T ? row[t + 1] : 0;
    const bool on = (cur & 127) != 0;
    const bool s = on && (t == 0 || (prev & 127) == 0 || (a.split && (cur & 128)));
    const bool l = on && (t + 1 == a.T || (next & 127) == 0 || (a.split && (next & 128)));
    const unsigned long long S = __ballot(s), L = __ballot(l);
    if (lane == 0) { a.starts[item] = S; a.lasts[item] = L; }
}

__global__ void __launch_bounds__(512) roll_prefix_kernel(RollArgs a) {
    __shared__ int sc[512];
    const int b = blockIdx.x, w = threadIdx.x;
    int c = 0;
    if (w < a.NW)
        for (int p = 0; p < 128; ++p) c += __popcll(a.lasts[((size_t)b * 128 + p) * a.NW + w]);
    sc[w] = c;
    __syncthreads();
    for (int o = 1; o < 512; o <<= 1) {
        const int add = w >= o ? sc[w - o] : 0;
        __syncthreads();
        sc[w] += add;
        __syncthreads();
    }
    if (w < a.NW) a.base[(size_t)b * a.NW + w] = sc[w] - c;
    if (w == 511) a.counts[b] = sc[511];
}

__global__ void __launch_bounds__(64) roll_emit_kernel(RollArgs a, int4* notes, int N) {
    __shared__ unsigned long long Lw[128];
    const int lane = threadIdx.x, w = blockIdx.x % a.NW, b = blockIdx.x / a.NW;
    const size_t rb = (size_t)b * 128;
    Lw[lane] = a.lasts[(rb + lane) * a.NW + w];
    Lw[lane + 64] = a.lasts[(rb + lane + 64) * a.NW + w];
    __syncthreads();
    int cnt = 0;
    for (int p = 0; p < 128; ++p) cnt += (int)((Lw[p] >> lane) & 1ull);
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    int slot = a.base[(size_t)b * a.NW + w] + incl - cnt;
    const int t = w * 64 + lane;
    for (int p = 0; p < 128 && cnt > 0; ++p) {
        if (!((Lw[p] >> lane) & 1ull)) continue;
        --cnt;
        const int my = slot++;
        if (my >= N) continue;
        const unsigned long long* S = a.starts + (rb + p) * a.NW;
        int start = 0;
        unsigned long long m = S[w] & (~0ull >> (63 - lane));
        for (int ww = w;;) {
            if (m) { start = ww * 64 + 63 - __clzll((long long)m); break; }
            if (--ww < 0) break;
            m = S[ww];
        }
        const int vel = a.plane[(rb + p) * a.T + start] & 127;
        notes[(size_t)b * N + my] = make_int4(p, start, t + 1, vel);
    }
}

constexpr int RR_THREADS = 256;

__global__ void __launch_bounds__(RR_THREADS) roll_render_kernel(const int4* notes, const long long* counts, int N, int width, const int* col0,
                                                                 unsigned char* out) {
    extern __shared__ unsigned rr_px[];                                  // [width + 1]: columns c0 - 1 .. c0 + width - 1
    const int pitch = blockIdx.x & 127, b = blockIdx.x >> 7, tid = threadIdx.x;
    int c0 = col0 ? col0[b] : 0;
    c0 = c0 < 0 ? 0 : c0 > (1 << 30) ? (1 << 30) : c0;
    for (int i = tid; i <= width; i += RR_THREADS) rr_px[i] = 0u;
    __syncthreads();
    long long cnt = counts[b];
    if (cnt > N) cnt = N;
    const int lo = c0 - 1, hi = c0 + width;                              // the window [lo, hi)
    for (int i = tid; i < (int)cnt; i += RR_THREADS) {
        const int4 nt = notes[(size_t)b * N + i];
        if (nt.x != pitch) continue;
        const unsigned key = (unsigned)(i + 1) << 8;
        const unsigned v = (unsigned)(nt.w < 0 ? 0 : nt.w > 255 ? 255 : nt.w);
        const int s = nt.y > lo ? nt.y : lo, e = nt.z < hi ? nt.z : hi;
        for (int t = s; t < e; ++t) atomicMax(&rr_px[t - lo], key | v);
        if (nt.y > 0 && nt.y - 1 >= lo && nt.y - 1 < hi) atomicMax(&rr_px[nt.y - 1 - lo], key);
    }
    __syncthreads();
    const size_t n = (size_t)128 * width;
    unsigned char* o = out + (size_t)b * 3 * n + (size_t)(127 - pitch) * width;
    for (int x = tid; x < width; x += RR_THREADS) {
        const int v = (int)(rr_px[x + 1] & 255u), pv = (int)(rr_px[x] & 255u);
        const int g = 2 * v < 255 ? 2 * v : 255;
        const bool red = v >= 11 && (c0 + x == 0 || pv <= 9);
        o[x] = (unsigned char)(red ? g : 0);
        o[n + x] = (unsigned char)(red ? 0 : g);
        o[2 * n + x] = 0;
    }
}

struct RollWs { size_t plane, starts, lasts, base, mm, total; };
static RollWs roll_ws(int B, int T) {
    const size_t NW = (size_t)(T + 63) / 64;
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    RollWs w;
    w.plane = 0;
    w.starts = up((size_t)B * 128 * T);
    w.lasts = w.starts + (size_t)B * 128 * NW * 8;
    w.base = w.lasts + (size_t)B * 128 * NW * 8;
    w.mm = w.base + up((size_t)B * NW * 4);
    w.total = w.mm + up((size_t)B * 8);
    return w;
}

static void roll_bind(RollArgs& a, void* ws_dev, int B, int T) {
    const RollWs w = roll_ws(B, T);
    char* p = static_cast<char*>(ws_dev);
    a.B = B; a.T = T; a.NW = (T + 63) / 64;
    a.plane = reinterpret_cast<unsigned char*>(p + w.plane);
    a.starts = reinterpret_cast<unsigned long long*>(p + w.starts);
    a.lasts = reinterpret_cast<unsigned long long*>(p + w.lasts);
    a.base = reinterpret_cast<int*>(p + w.base);
    a.mm = reinterpret_cast<unsigned*>(p + w.mm);
}

}  // namespace fc

using namespace fc;

extern "C" {

int64_t fc_pianoroll_workspace_bytes(int batch, int columns) {
    if (batch < 1 || columns < 1 || columns > FC_ROLL_MAX_COLUMNS || (long long)batch * columns > (1ll << 31)) return -1;
    return (int64_t)roll_ws(batch, columns).total;
}

int fc_pianoroll_scan(const void* images_dev, int is_float, int batch, int height, int width, int layout, int require_onsets, int separators,
                      int split_on_onsets, void* ws_dev, int64_t* counts_out_dev, void* stream) {
    if (!images_dev || !ws_dev || !counts_out_dev) return fail(FC_E_ARG, "fc_pianoroll_scan: null argument");
    if ((reinterpret_cast<uintptr_t>(ws_dev) & 15) || (reinterpret_cast<uintptr_t>(counts_out_dev) & 7) ||
        (is_float && (reinterpret_cast<uintptr_t>(images_dev) & 3)))
        return fail(FC_E_ARG, "fc_pianoroll_scan: a misaligned pointer (workspace 16, counts 8, float images 4 bytes)");
    if (batch < 1 || height < 128 || width < 1 || height % 128) return fail(FC_E_SHAPE, "fc_pianoroll_scan: images are [B,3,128 S,W]");
    if (separators < 0) return fail(FC_E_ARG, "fc_pianoroll_scan: separators must be >= 0");
    RollArgs a = {};
    long long T;
    if (layout == FC_ROLL_STRIPS) {
        T = (long long)(height / 128) * width;
        a.sq = 0; a.period = width;
    } else if (layout == FC_ROLL_SQUARE) {
        if (height != 256 || width != 256) return fail(FC_E_SHAPE, "fc_pianoroll_scan: the square layout is 256 x 256");
        T = 512;
        a.sq = 1; a.period = 512;
    } else if (layout == FC_ROLL_GRID) {
        if (height != 2048 || width != 2048) return fail(FC_E_SHAPE, "fc_pianoroll_scan: the grid layout is 2048 x 2048");
        T = 32768;
        a.sq = 8; a.period = 2048;
    } else {
        return fail(FC_E_ARG, "fc_pianoroll_scan: unknown layout");
    }
    if (T > FC_ROLL_MAX_COLUMNS) return fail(FC_E_SHAPE, "fc_pianoroll_scan: more than FC_ROLL_MAX_COLUMNS columns per roll");
    if ((long long)batch * T > (1ll << 31)) return fail(FC_E_SHAPE, "fc_pianoroll_scan: more than 2^31 columns in all");
    roll_bind(a, ws_dev, batch, (int)T);
    a.img = images_dev; a.H = height; a.W = width;
    a.require = require_onsets != 0; a.sep = separators; a.split = split_on_onsets != 0;
    a.counts = reinterpret_cast<long long*>(counts_out_dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (is_float) {
        const long long per = 3ll * height * width;
        const long long want = (per + RL_THREADS * 16 - 1) / (RL_THREADS * 16);
        FC_HIP(hipMemsetAsync(const_cast<unsigned*>(a.mm), 0, sizeof(unsigned) * 2 * (size_t)batch, s));
        hipLaunchKernelGGL(roll_minmax_kernel, dim3((unsigned)(want < 256 ? want : 256), batch), dim3(RL_THREADS), 0, s,
                           static_cast<const float*>(images_dev), per, const_cast<unsigned*>(a.mm));
        FC_HIP(hipGetLastError());
    }
    const int wpb = RL_THREADS / 64;
    const long long items = (long long)batch * 128 * ((a.NW + RL_CHUNK - 1) / RL_CHUNK);
    hipLaunchKernelGGL(is_float ? roll_filter_kernel<true> : roll_filter_kernel<false>, dim3((unsigned)((items + wpb - 1) / wpb)),
                       dim3(RL_THREADS), 0, s, a);
    FC_HIP(hipGetLastError());
    const long long words = (long long)batch * 128 * a.NW;
    hipLaunchKernelGGL(roll_masks_kernel, dim3((unsigned)((words + wpb - 1) / wpb)), dim3(RL_THREADS), 0, s, a);
    FC_HIP(hipGetLastError());
    hipLaunchKernelGGL(roll_prefix_kernel, dim3(batch), dim3(512), 0, s, a);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

int fc_pianoroll_emit(const void* ws_dev, int batch, int columns, int32_t* notes_out_dev, int max_notes, void* stream) {
    if (!ws_dev || (max_notes > 0 && !notes_out_dev)) return fail(FC_E_ARG, "fc_pianoroll_emit: null argument");
    if ((reinterpret_cast<uintptr_t>(ws_dev) & 15) || (reinterpret_cast<uintptr_t>(notes_out_dev) & 15))
        return fail(FC_E_ARG, "fc_pianoroll_emit: the workspace and the notes must be 16-byte aligned");
    if (batch < 1 || columns < 1 || columns > FC_ROLL_MAX_COLUMNS || (long long)batch * columns > (1ll << 31) || max_notes < 0)
        return fail(FC_E_SHAPE, "fc_pianoroll_emit: batch >= 1, 1 <= columns <= FC_ROLL_MAX_COLUMNS, max_notes >= 0");
    if ((long long)batch * max_notes > (1ll << 28)) return fail(FC_E_SHAPE, "fc_pianoroll_emit: more than 2^28 note slots");
    if (max_notes == 0) return FC_OK;
    RollArgs a = {};
    roll_bind(a, const_cast<void*>(ws_dev), batch, columns);
    hipStream_t s = static_cast<hipStream_t>(stream);
    FC_HIP(hipMemsetAsync(notes_out_dev, 0xff, sizeof(int32_t) * 4 * (size_t)batch * max_notes, s));
    hipLaunchKernelGGL(roll_emit_kernel, dim3((unsigned)(batch * a.NW)), dim3(64), 0, s, a, reinterpret_cast<int4*>(notes_out_dev), max_notes);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

int fc_pianoroll_render(const int32_t* notes_dev, const int64_t* counts_dev, int batch, int max_notes, int width, const int32_t* col0_dev,
                        uint8_t* images_out_dev, void* stream) {
    if (!counts_dev || !images_out_dev || (max_notes > 0 && !notes_dev)) return fail(FC_E_ARG, "fc_pianoroll_render: null argument");
    if ((reinterpret_cast<uintptr_t>(notes_dev) & 15) || (reinterpret_cast<uintptr_t>(counts_dev) & 7) || (reinterpret_cast<uintptr_t>(col0_dev) & 3))
        return fail(FC_E_ARG, "fc_pianoroll_render: a misaligned pointer (notes 16, counts 8, col0 4 bytes)");
    if (batch < 1 || batch > (1 << 20) || width < 1 || width > FC_ROLL_MAX_WIDTH || max_notes < 0 || max_notes >= (1 << 23))
        return fail(FC_E_SHAPE, "fc_pianoroll_render: 1 <= batch <= 2^20, 1 <= width <= FC_ROLL_MAX_WIDTH, 0 <= max_notes < 2^23");
    hipLaunchKernelGGL(roll_render_kernel, dim3((unsigned)batch * 128), dim3(RR_THREADS), sizeof(unsigned) * (width + 1),
                       static_cast<hipStream_t>(stream), reinterpret_cast<const int4*>(notes_dev), reinterpret_cast<const long long*>(counts_dev),
                       max_notes, width, col0_dev, images_out_dev);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

}  // extern "C"
