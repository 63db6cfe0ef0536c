// Pre-encoding augmentation from a resident image pool: upstream's image_transforms and midi_transforms (flocoder/data.py:49-111) as one
// launch each, straight into the fp32 NCHW tensor the codec's encode reads.  flocoder_amd/noise.py (augment_image_field, augment_midi_field)
// defines the output; the random draws are made there, on the host, and arrive as one row of integers per sample, so nothing here draws
// and every choice of a source pixel is the same integer arithmetic as the definition's.
//
// Images.  Row = (source, a0..a5, crop left, crop top, crop side, box x0, box y0, box w, box h, flip, 0).  The rotated image R is virtual:
// R[Y][X] = source[(a3 X + a4 Y + a5) >> 16][(a0 X + a1 Y + a2) >> 16] (Q16, 64-bit), `fill` outside.  Output pixel (i, j) of the box
// resized to S x S is sum_y sum_x ny(y) nx(x) R[top + y][left + x] / (Ny Nx) with PIL's antialiased bilinear taps in integers: for an axis
// with origin o, extent e and D = 2 max(S, e), c_j = 2 S o + (2 j + 1) e, taps lo_j <= x < hi_j (clamped to the crop), numerator
// n(x) = max(0, D - |(2 x + 1) S - c_j|), N = their sum.  Per output column and row only (lo, hi, c, 1 / N) are kept -- 16 of each per tile
// in LDS; a numerator is three integer operations at the tap -- so a window of any size needs no weight table.  The numerators and the
// bytes are integers below 2^24, their products exact in fp32; what rounds are the running sums (all terms non-negative) and the final
// scaling: the error grows with taps_x + taps_y, not with their product.
//
// Shape: a workgroup of four waves per 16 x 16 output tile, a lane per output pixel; four adjacent lanes then exchange their values so that
// three of them store one channel's four columns as a float4 each (one value per lane when S is no multiple of 4).  The tile's taps
// span a rectangle of the crop; when it has at most FC_AUG_LDS_PIXELS pixels the workgroup stages R over that rectangle in LDS once, four
// bytes per pixel (r, g, b, outside flag), so the rotation's gather runs once per pixel and the taps are LDS reads; a larger window (a
// large source shrunk to a small size) reads the source through L2 at every tap.  The outside flag gathers the weight that fell outside
// the source, which is multiplied by `fill` at the end, so `fill` need not be a byte.
//
// MIDI.  Row = (source, shift x, shift y, crop left, crop top, 0, 0, 0): a translation with zero fill, a crop, byte / 255 in fp32 (a
// correctly rounded division), optionally the clamped channel sum and the >= threshold gate: integers and one fp32 compare, equal to the
// host form in every bit.  A lane per four adjacent columns.
#include <math.h>

#include "common.h"

namespace fc {

constexpr int AG_TILE = 16, AG_THREADS = AG_TILE * AG_TILE, AG_MIDI_THREADS = 256;

struct AugConst { float mean[3], std[3], fill_byte[3]; };

struct AugSource { const unsigned char* p; int H, W, C; };

// a sample's source: an index outside the table, or a channel count the kernels do not read, is a source of no pixels
__device__ __forceinline__ AugSource aug_source(const unsigned char* pool, const longlong4* table, int n_sources, int src) {
    AugSource s = {pool, 0, 0, 1};
    if (src >= 0 && src < n_sources) {
        const longlong4 e = table[src];
        if ((e.w == 1 || e.w == 3) && e.x >= 0 && e.y > 0 && e.z > 0 && e.y <= FC_AUG_MAX_SIDE && e.z <= FC_AUG_MAX_SIDE)
            s = {pool + e.x, (int)e.y, (int)e.z, (int)e.w};
    }
    return s;
}

struct AugRot { long long a0, a1, a2, a3, a4, a5; };

// R[Y][X] as r | g << 8 | b << 16, or 1 << 24 outside the source
__device__ __forceinline__ unsigned aug_fetch(const AugSource& s, const AugRot& m, int X, int Y) {
    const long long sx = (m.a0 * X + m.a1 * Y + m.a2) >> 16, sy = (m.a3 * X + m.a4 * Y + m.a5) >> 16;
    if (sx < 0 || sx >= s.W || sy < 0 || sy >= s.H) return 1u << 24;
    const unsigned char* p = s.p + ((size_t)sy * s.W + (size_t)sx) * s.C;
    const unsigned r = p[0];
    return s.C == 3 ? r | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) : r * 0x010101u;
}

// one output pixel: the three channels, normalised.  An empty tap range (a row or column past the image) gives a value nobody stores.
template <bool LDS>
__device__ __forceinline__ void aug_pixel(float v[3], const AugConst& k, const AugSource& s, const AugRot& m, const unsigned* win, int S, int left,
                                          int top, int wx0, int wy0, int ww, int dx, int dy, const int* p_lo, const int* p_hi, const int* p_c,
                                          const float* p_inv, int col, int r) {
    const int ylo = p_lo[AG_TILE + r], yhi = p_hi[AG_TILE + r], yc = p_c[AG_TILE + r];
    const int xlo = p_lo[col], xhi = p_hi[col], xc = p_c[col];
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, af = 0.f;
    for (int y = ylo; y < yhi; ++y) {
        const int ady = (2 * y + 1) * S - yc;
        const int ny = dy - (ady < 0 ? -ady : ady);
        float r0 = 0.f, r1 = 0.f, r2 = 0.f, rf = 0.f;
        for (int x = xlo; x < xhi; ++x) {
            const int adx = (2 * x + 1) * S - xc;
            const int nx = dx - (adx < 0 ? -adx : adx);
            const unsigned p = LDS ? win[(y - wy0) * ww + (x - wx0)] : aug_fetch(s, m, left + x, top + y);
            const float w = (float)(nx < 0 ? 0 : nx);
            r0 += w * (float)(p & 255u);
            r1 += w * (float)((p >> 8) & 255u);
            r2 += w * (float)((p >> 16) & 255u);
            rf += w * (float)(p >> 24);
        }
        const float wy = (float)(ny < 0 ? 0 : ny);
        a0 += wy * r0; a1 += wy * r1; a2 += wy * r2; af += wy * rf;
    }
    const float sc = p_inv[col] * p_inv[AG_TILE + r];
    v[0] = (((a0 + k.fill_byte[0] * af) * sc) / 255.f - k.mean[0]) / k.std[0];
    v[1] = (((a1 + k.fill_byte[1] * af) * sc) / 255.f - k.mean[1]) / k.std[1];
    v[2] = (((a2 + k.fill_byte[2] * af) * sc) / 255.f - k.mean[2]) / k.std[2];
}

__global__ void __launch_bounds__(AG_THREADS) augment_images_kernel(float* out, const unsigned char* pool, const longlong4* table, int n_sources,
                                                                    const int* stab, int S, int tiles, AugConst k, int vec) {
    __shared__ unsigned win[FC_AUG_LDS_PIXELS];
    __shared__ int p_lo[2 * AG_TILE], p_hi[2 * AG_TILE], p_c[2 * AG_TILE];  // [0, 16): the tile's columns, [16, 32): its rows
    __shared__ float p_inv[2 * AG_TILE];

    const int tid = threadIdx.x;
    const int b = blockIdx.x / (tiles * tiles), t = blockIdx.x % (tiles * tiles);
    const int ox0 = (t % tiles) * AG_TILE, oy0 = (t / tiles) * AG_TILE;
    const int* row = stab + (size_t)b * FC_AUG_IMAGE_WORDS;
    const AugSource s = aug_source(pool, table, n_sources, row[0]);
    const AugRot m = {row[1], row[2], row[3], row[4], row[5], row[6]};
    // what the loops and the coordinates are bounded by is made sane here, whatever the row holds: the crop's corner within a side's
    // length of the origin, 1 <= side, 1 <= box <= side, the box inside the crop
    const int left = min(max(row[7], -FC_AUG_MAX_SIDE), FC_AUG_MAX_SIDE), top = min(max(row[8], -FC_AUG_MAX_SIDE), FC_AUG_MAX_SIDE);
    const int side = min(max(row[9], 1), FC_AUG_MAX_SIDE);
    const int bw = min(max(row[12], 1), side), bh = min(max(row[13], 1), side);
    const int bx = min(max(row[10], 0), side - bw), by = min(max(row[11], 0), side - bh);
    const bool flip = row[14] != 0;
    const int dx = 2 * max(S, bw), dy = 2 * max(S, bh);

    if (tid < 2 * AG_TILE) {
        const bool is_y = tid >= AG_TILE;
        const int o = is_y ? oy0 + tid - AG_TILE : ox0 + tid;               // the output row / column
        int lo = 0, hi = 0, c = 0;
        float inv = 0.f;
        if (o < S) {
            const int j = (!is_y && flip) ? S - 1 - o : o;
            const int e = is_y ? bh : bw, d = is_y ? dy : dx;
            c = 2 * S * (is_y ? by : bx) + (2 * j + 1) * e;
            lo = c - d + S < 0 ? 0 : (c - d + S) / (2 * S);
            hi = min(side, (c + d + S) / (2 * S));
            long long n = 0;
            for (int x = lo; x < hi; ++x) {
                const int a = (2 * x + 1) * S - c;
                n += max(0, d - (a < 0 ? -a : a));
            }
            inv = 1.f / (float)n;                                           // n >= 1: the tap under the centre has a positive numerator
        }
        p_lo[tid] = lo; p_hi[tid] = hi; p_c[tid] = c; p_inv[tid] = inv;
    }
    __syncthreads();

    int wx0 = side, wx1 = 0, wy0 = side, wy1 = 0;                           // the rectangle of the crop this tile's taps span
    for (int i = 0; i < AG_TILE; ++i) {
        if (ox0 + i < S) { wx0 = min(wx0, p_lo[i]); wx1 = max(wx1, p_hi[i]); }
        if (oy0 + i < S) { wy0 = min(wy0, p_lo[AG_TILE + i]); wy1 = max(wy1, p_hi[AG_TILE + i]); }
    }
    const int ww = wx1 - wx0, wh = wy1 - wy0;
    const bool staged = (long long)ww * wh <= FC_AUG_LDS_PIXELS;            // the same in every lane
    if (staged) {
        const int n = ww * wh;
        for (int i0 = tid; i0 < n; i0 += 4 * AG_THREADS) {                  // four independent gathers in flight per lane
            unsigned p[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + u * AG_THREADS, y = i / ww, x = i - y * ww;
                p[u] = i < n ? aug_fetch(s, m, left + wx0 + x, top + wy0 + y) : 0u;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i0 + u * AG_THREADS < n) win[i0 + u * AG_THREADS] = p[u];
        }
        __syncthreads();
    }
    const int col = tid & (AG_TILE - 1), r = tid >> 4, ox = ox0 + col, oy = oy0 + r;
    float v[3];
    if (staged)
        aug_pixel<true>(v, k, s, m, win, S, left, top, wx0, wy0, ww, dx, dy, p_lo, p_hi, p_c, p_inv, col, r);
    else
        aug_pixel<false>(v, k, s, m, win, S, left, top, wx0, wy0, ww, dx, dy, p_lo, p_hi, p_c, p_inv, col, r);
    const bool live = ox < S && oy < S;
    if (vec) {
        // S a multiple of 4: four adjacent lanes hold four adjacent columns of one row, all inside the image or all outside.  Lane c < 3 of
        // the four collects channel c from its neighbours and stores it as one float4; every lane of the wave takes part in the exchange.
        const int lane = tid & 63, q0 = lane & ~3, c = lane & 3;
        float g[3][4];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
#pragma unroll
            for (int i = 0; i < 4; ++i) g[ch][i] = __shfl(v[ch], q0 + i);
        if (live && c < 3) {
            const float4 f = c == 0 ? make_float4(g[0][0], g[0][1], g[0][2], g[0][3])
                           : c == 1 ? make_float4(g[1][0], g[1][1], g[1][2], g[1][3]) : make_float4(g[2][0], g[2][1], g[2][2], g[2][3]);
            *reinterpret_cast<float4*>(out + (((size_t)b * 3 + c) * S + oy) * S + (ox & ~3)) = f;
        }
    } else if (live) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out[(((size_t)b * 3 + ch) * S + oy) * S + ox] = v[ch];
    }
}

__global__ void __launch_bounds__(AG_MIDI_THREADS) augment_midi_kernel(float* out, const unsigned char* pool, const longlong4* table, int n_sources,
                                                                       const int* stab, long long total, int S, int quads, int oc, int gray,
                                                                       float threshold, int vec) {
    const long long item = (long long)blockIdx.x * AG_MIDI_THREADS + threadIdx.x;       // (sample, row, four columns)
    if (item >= total) return;
    const int qx = (int)(item % quads), y = (int)((item / quads) % S), b = (int)(item / ((long long)quads * S));
    const int* row = stab + (size_t)b * FC_AUG_MIDI_WORDS;
    const AugSource s = aug_source(pool, table, n_sources, row[0]);
    const long long sy = (long long)y + row[4] - row[2], sx0 = (long long)qx * 4 + row[3] - row[1];
    float v[3][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long sx = sx0 + i;
        float u0 = 0.f, u1 = 0.f, u2 = 0.f;
        if (sy >= 0 && sy < s.H && sx >= 0 && sx < s.W) {
            const unsigned char* p = s.p + ((size_t)sy * s.W + (size_t)sx) * s.C;
            u0 = (float)p[0] / 255.f;
            u1 = s.C == 3 ? (float)p[1] / 255.f : u0;
            u2 = s.C == 3 ? (float)p[2] / 255.f : u0;
        }
        if (gray) {
            const float g = s.C == 3 ? (u0 + u1) + u2 : u0;
            u0 = u1 = u2 = fminf(fmaxf(g, 0.f), 1.f);
        }
        if (threshold > 0.f) {
            u0 = u0 >= threshold ? 1.f : 0.f; u1 = u1 >= threshold ? 1.f : 0.f; u2 = u2 >= threshold ? 1.f : 0.f;
        }
        v[0][i] = u0; v[1][i] = u1; v[2][i] = u2;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c >= oc) break;
        float* o = out + (((size_t)b * oc + c) * S + y) * S + (size_t)qx * 4;
        if (vec) {
            *reinterpret_cast<float4*>(o) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (qx * 4 + i < S) o[i] = v[c][i];
        }
    }
}

static int aug_check(const char* fn, const void* out, const void* pool, const void* table, int n_sources, const void* stab, int batch, int size) {
    if (!out || !pool || !table || !stab) return fail(FC_E_ARG, std::string(fn) + ": null argument");
    if (reinterpret_cast<uintptr_t>(table) & 15) return fail(FC_E_ARG, std::string(fn) + ": the source table must be 16-byte aligned");
    if (n_sources < 1) return fail(FC_E_ARG, std::string(fn) + ": the pool holds no source");
    if (batch < 1) return fail(FC_E_SHAPE, std::string(fn) + ": batch must be positive");
    if (size < FC_AUG_MIN_SIZE || size > FC_AUG_MAX_SIZE) return fail(FC_E_SHAPE, std::string(fn) + ": size must lie in [16, 1024]");
    return FC_OK;
}

}  // namespace fc

using namespace fc;

extern "C" {

int fc_augment_images(float* out_dev, const uint8_t* pool_dev, const int64_t* table_dev, int n_sources, const int* sample_table_dev, int batch,
                      int size, const float* mean_host, const float* std_host, const float* fill_host, void* stream) {
    FC_TRY(aug_check("fc_augment_images", out_dev, pool_dev, table_dev, n_sources, sample_table_dev, batch, size));
    if (!mean_host || !std_host || !fill_host) return fail(FC_E_ARG, "fc_augment_images: null mean, std or fill");
    AugConst k;
    for (int c = 0; c < 3; ++c) {
        if (!std::isfinite(std_host[c]) || !(std_host[c] > 0.f)) return fail(FC_E_ARG, "fc_augment_images: std must be finite and positive");
        if (!std::isfinite(mean_host[c]) || !std::isfinite(fill_host[c])) return fail(FC_E_ARG, "fc_augment_images: mean and fill must be finite");
        k.mean[c] = mean_host[c];
        k.std[c] = std_host[c];
        k.fill_byte[c] = (float)(255.0 * ((double)fill_host[c] * (double)std_host[c] + (double)mean_host[c]));
    }
    const int tiles = cdiv(size, AG_TILE);
    const long long blocks = (long long)batch * tiles * tiles;
    if (blocks > 0x7fffffffLL) return fail(FC_E_SHAPE, "fc_augment_images: batch x tiles exceeds one launch");
    const int vec = (size & 3) == 0 && (reinterpret_cast<uintptr_t>(out_dev) & 15) == 0;
    hipLaunchKernelGGL(augment_images_kernel, dim3((unsigned)blocks), dim3(AG_THREADS), 0, static_cast<hipStream_t>(stream), out_dev, pool_dev,
                       reinterpret_cast<const longlong4*>(table_dev), n_sources, sample_table_dev, size, tiles, k, vec);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

int fc_augment_midi(float* out_dev, const uint8_t* pool_dev, const int64_t* table_dev, int n_sources, const int* sample_table_dev, int batch,
                    int size, int out_channels, int gray, float threshold, void* stream) {
    FC_TRY(aug_check("fc_augment_midi", out_dev, pool_dev, table_dev, n_sources, sample_table_dev, batch, size));
    if (out_channels != 1 && out_channels != 3) return fail(FC_E_SHAPE, "fc_augment_midi: out_channels is 1 or 3");
    if (!std::isfinite(threshold)) return fail(FC_E_ARG, "fc_augment_midi: threshold must be finite");
    const int quads = cdiv(size, 4);
    const long long total = (long long)batch * size * quads;
    const long long blocks = (total + AG_MIDI_THREADS - 1) / AG_MIDI_THREADS;
    if (blocks > 0x7fffffffLL) return fail(FC_E_SHAPE, "fc_augment_midi: batch x size^2 exceeds one launch");
    const int vec = (size & 3) == 0 && (reinterpret_cast<uintptr_t>(out_dev) & 15) == 0;
    hipLaunchKernelGGL(augment_midi_kernel, dim3((unsigned)blocks), dim3(AG_MIDI_THREADS), 0, static_cast<hipStream_t>(stream), out_dev, pool_dev,
                       reinterpret_cast<const longlong4*>(table_dev), n_sources, sample_table_dev, total, size, quads, out_channels, gray != 0 ? 1 : 0,
                       threshold, vec);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

}  // extern "C"
