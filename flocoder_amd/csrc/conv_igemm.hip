// Implicit-GEMM convolution for gfx950 on the exact-fp32 matrix pipe (v_mfma_f32_32x32x2_f32).
//
//   out[b,y,x,:] = bias + sum_{ky,kx,c} W[ky,kx,c,:] * X(b, y*s-p+ky, x*s-p+kx, c)
//
// X is the *logical* input: up to two NHWC tensors concatenated along C, each optionally passed through
// "GroupNorm affine (+FiLM) (+SiLU)" while it is staged, optionally nearest-x2 upsampled -- so torch.cat,
// nn.Upsample, the space-to-depth Rearrange, GroupNorm, the scale/shift modulation and SiLU of the
// reference's Block/ResnetBlock (unet.py:42-96) never exist as separate passes over HBM.
//
// Work decomposition (one 256-thread workgroup = 4 wave64):
//   M tile = TB samples x TH rows x TW cols of output pixels (BM = 32*MT*WM of them), N tile = BN output
//   channels, K = KS*KS*Cin walked in chunks of CC input channels.  Per chunk the workgroup stages
//     patch[TB][PH][PW][CC(+1 pad)]   the input window incl. halo, transformed, zero outside the image
//     wl[KS*KS][CC][BN]               the weight slab
//   in LDS once; the 9 taps then read the patch at constant offsets, so each input element is fetched
//   from L2/HBM once per (tile, chunk) rather than once per tap.  Waves are laid out WM x WN x WK: WK > 1
//   splits the K steps of a chunk across waves (small-M layers would otherwise leave 3 of 4 SIMDs idle
//   behind one wave's 64-cycle MFMA issue), partial accumulators meet in LDS in the epilogue.
//   MFMA operand maps (cdna_hip_programming.md 3): A lane l = A[row l&31][k l>>5], B lane l = B[k l>>5][col l&31],
//   D reg r = D[row (r&3)+8*(r>>2)+4*(l>>5)][col l&31].
//
// Epilogue: + bias, per-tile GroupNorm partials (mean, M2) of the result written without atomics, optional
// SiLU, optional residual add, optional second accumulator = 1x1 projection of the centre tap
// (ResnetBlock.res_conv shares conv1's staged input).
#include <cstdlib>
#include <string>

#include "conv_dev.h"

namespace fc {

template <int WM, int WN, int WK, int MT, int NT, int CC>
__global__ void __launch_bounds__(256) conv_igemm_kernel(const ConvDev p) {
    constexpr int BN = 32 * NT * WN, CS = CC + 1, KSTEPS = CC / 2, KPW = KSTEPS / WK, Q = CC / 4;
    static_assert(WM * WN * WK == 4, "4 waves per workgroup");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const ConvArgs& a = p.a;
    int* pixoff = reinterpret_cast<int*>(smem + p.o_pixoff);
    int* pixtb = reinterpret_cast<int*>(smem + p.o_pixtb);
    float* gstat = smem + p.o_gstat;
    float2* aff = reinterpret_cast<float2*>(smem + p.o_aff);
    float* patch = smem + p.o_patch;
    float* wl = smem + p.o_wl;
    float* wres = smem + p.o_wres;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int wk = wave % WK, wn = (wave / WK) % WN, wm = wave / (WK * WN);

    const int bid = xcd_remap(blockIdx.x, p.nblocks);
    const int nt_i = bid % p.ntiles, mt_i = bid / p.ntiles;
    const int tx = mt_i % p.tiles_x, ty = (mt_i / p.tiles_x) % p.tiles_y, bg = mt_i / (p.tiles_x * p.tiles_y);
    const int TW = 1 << p.TWl, TH = 1 << p.THl;
    const int b0 = bg * p.TB, y0 = ty * TH, x0 = tx * TW, n0 = nt_i * BN;
    const int KS = a.KS, KK = KS * KS, PW = p.PW, PHW = p.PH * p.PW;
    const int C0 = a.s0.C, C1 = a.s1.C, Cin = a.Cin, Cout = a.Cout;
    const bool has_res = a.res_out != nullptr;

    // ---- one-time tables: where each patch pixel lives in the source, and the GroupNorm moments ----
    {
        const int Hin = a.Hs << a.ups, Win = a.Ws << a.ups;
        for (int i = tid; i < p.P; i += 256) {
            const int tb = i / PHW, r = i - tb * PHW, py = r / PW, px = r - py * PW;
            const int iy = y0 * a.stride - (a.pad_y >= 0 ? a.pad_y : a.pad) + py, ix = x0 * a.stride - (a.pad_x >= 0 ? a.pad_x : a.pad) + px, b = b0 + tb;
            int off = -1;
            if (b < a.B && iy >= 0 && iy < Hin && ix >= 0 && ix < Win) off = (b * a.Hs + (iy >> a.ups)) * a.Ws + (ix >> a.ups);
            pixoff[i] = off;
            pixtb[i] = tb;
        }
        if (p.any_xf) {
            const int G0 = a.s0.xf.mode ? a.s0.xf.G : 0, G1 = a.s1.xf.mode ? a.s1.xf.G : 0;
            for (int i = tid; i < p.TB * (G0 + G1); i += 256) {
                const bool first = i < p.TB * G0;
                const SrcXform& xf = first ? a.s0.xf : a.s1.xf;
                const int j = first ? i : i - p.TB * G0;
                const int tb = j / xf.G, g = j - tb * xf.G, b = b0 + tb;
                float mean = 0.f, rstd = 0.f;
                if (b < a.B) {
                    const float* sp = xf.stats + (size_t)(b * xf.G + g) * xf.T * 2;
                    float sm = 0.f;
                    for (int t = 0; t < xf.T; ++t) sm += sp[2 * t];
                    mean = sm / (float)xf.T;
                    float m2 = 0.f, dv = 0.f;
                    for (int t = 0; t < xf.T; ++t) {
                        const float d = sp[2 * t] - mean;
                        m2 += sp[2 * t + 1];
                        dv += d * d;
                    }
                    const float var = (m2 + xf.n_t * dv) / (xf.n_t * (float)xf.T);
                    rstd = 1.0f / sqrtf(var + xf.eps);
                }
                gstat[2 * i] = mean;
                gstat[2 * i + 1] = rstd;
            }
            __syncthreads();   // step (a) of the first chunk reads gstat from other waves
        }
    }

    // ---- per-lane operand bases ----
    int abase[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int m = (wm * MT + mt) * 32 + l31;
        const int tw = m & (TW - 1), th = (m >> p.TWl) & (TH - 1), tb = m >> (p.TWl + p.THl);
        abase[mt] = (tb * PHW + th * a.stride * PW + tw * a.stride) * CS + half;
    }
    const int bbase = half * BN + wn * NT * 32 + l31;
    const int kk0 = wk * KPW;

    f32x16 acc[MT][NT], accr[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[mt][nt][r] = 0.f; accr[mt][nt][r] = 0.f; }

    const float* wbase = a.w + (size_t)b0 * a.w_batch_stride;

    for (int c0 = 0; c0 < Cin; c0 += CC) {
        // (a) per-(sample, channel) affine of this chunk:  x -> A*x + B  == GroupNorm, FiLM folded in
        if (p.any_xf) {
            const int G0n = a.s0.xf.mode ? a.s0.xf.G : 0;
            for (int i = tid; i < p.TB * CC; i += 256) {
                const int tb = i / CC, c = c0 + (i - tb * CC), b = b0 + tb;
                float A = 1.f, Bv = 0.f;
                if (c < Cin && b < a.B) {
                    const bool first = c < C0;
                    const SrcXform& xf = first ? a.s0.xf : a.s1.xf;
                    if (xf.mode) {
                        const int cs = first ? c : c - C0, Cs = first ? C0 : C1;
                        const int g = cs / (Cs / xf.G);
                        const float* gs = gstat + 2 * ((first ? 0 : p.TB * G0n) + tb * xf.G + g);
                        A = gs[1] * xf.gamma[cs];
                        Bv = xf.beta[cs] - gs[0] * A;
                        if (xf.ss) {
                            const float sc = xf.ss[(size_t)b * xf.ss_stride + cs] + 1.0f;
                            const float sh = xf.ss[(size_t)b * xf.ss_stride + Cs + cs];
                            A *= sc;
                            Bv = Bv * sc + sh;
                        }
                    }
                }
                aff[i] = make_float2(A, Bv);
            }
        }
        __syncthreads();  // previous chunk's MFMAs are done with patch/wl; aff + tables visible

        // (b) stage the input window ...
        for (int e = tid; e < p.P * Q; e += 256) {
            const int pix = e / Q, q = e - pix * Q, c = c0 + 4 * q;
            const int po = pixoff[pix];
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (po >= 0 && c < Cin) {
                const bool first = c < C0;
                v = first ? *reinterpret_cast<const float4*>(a.s0.p + (size_t)po * C0 + c)
                          : *reinterpret_cast<const float4*>(a.s1.p + (size_t)po * C1 + (c - C0));
                if (p.any_xf) {
                    const float2* ab = aff + pixtb[pix] * CC + 4 * q;
                    v.x = ab[0].x * v.x + ab[0].y;
                    v.y = ab[1].x * v.y + ab[1].y;
                    v.z = ab[2].x * v.z + ab[2].y;
                    v.w = ab[3].x * v.w + ab[3].y;
                    if (first ? p.act0 : p.act1) { v.x = silu_f(v.x); v.y = silu_f(v.y); v.z = silu_f(v.z); v.w = silu_f(v.w); }
                }
            }
            float* d = patch + pix * CS + 4 * q;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        // ... and the weight slab [tap][c][BN]
        for (int e = tid; e < KK * CC * (BN / 4); e += 256) {
            const int n4 = e % (BN / 4), c = (e / (BN / 4)) % CC, tap = e / (BN / 4 * CC);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c0 + c < Cin && n0 + 4 * n4 < Cout)
                v = *reinterpret_cast<const float4*>(wbase + ((size_t)tap * Cin + c0 + c) * Cout + n0 + 4 * n4);
            *reinterpret_cast<float4*>(wl + (tap * CC + c) * BN + 4 * n4) = v;
        }
        if (has_res) {
            for (int e = tid; e < CC * (BN / 4); e += 256) {
                const int n4 = e % (BN / 4), c = e / (BN / 4);
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c0 + c < Cin && n0 + 4 * n4 < Cout)
                    v = *reinterpret_cast<const float4*>(a.res_w + (size_t)(c0 + c) * Cout + n0 + 4 * n4);
                *reinterpret_cast<float4*>(wres + c * BN + 4 * n4) = v;
            }
        }
        __syncthreads();

        // (c) MFMA over taps x this wave's K steps
        for (int ky = 0; ky < KS; ++ky) {
            for (int kx = 0; kx < KS; ++kx) {
                const int tapoff = (ky * PW + kx) * CS;
                const float* wt = wl + (ky * KS + kx) * CC * BN + bbase;
#pragma unroll
                for (int kk = 0; kk < KPW; ++kk) {
                    const int k = 2 * (kk0 + kk);
                    float av[MT], bv[NT];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) av[mt] = patch[abase[mt] + tapoff + k];
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) bv[nt] = wt[k * BN + nt * 32];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt)
                            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
                }
                if (has_res && ky == a.pad && kx == a.pad) {
#pragma unroll
                    for (int kk = 0; kk < KPW; ++kk) {
                        const int k = 2 * (kk0 + kk);
                        float av[MT], bv[NT];
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) av[mt] = patch[abase[mt] + tapoff + k];
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) bv[nt] = wres[(k + half) * BN + wn * NT * 32 + l31 + nt * 32];
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                            for (int nt = 0; nt < NT; ++nt)
                                accr[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt], bv[nt], accr[mt][nt], 0, 0, 0);
                    }
                }
            }
        }
    }

    conv_epilogue<WM, WN, WK, MT, NT>(p, acc, accr, smem, tid, lane, wave, b0, y0, x0, n0, tx, ty);
}

// ---------------------------------------------------------------------------------------------------
// The synchronous kernel's instantiation of every tile that has one (conv_dev.h kConvTiles): conv_init() and conv_launch() both ask here.
typedef void (*SyncKernel)(const ConvDev);
template <int TILE>
static constexpr SyncKernel sync_kernel() {
    constexpr ConvTileDef t = kConvTiles[TILE];
    if constexpr (t.CCs != 0) return &conv_igemm_kernel<t.WM, t.WN, t.WK, t.MT, t.NT, t.CCs>;
    else return nullptr;
}
static const SyncKernel kSyncKernels[TILE_COUNT] = {sync_kernel<TILE_M128N32>(), sync_kernel<TILE_M128N64>(), sync_kernel<TILE_M64N32K2>(),
                                                    sync_kernel<TILE_M32N32K4>(), sync_kernel<TILE_M64N64K2>(), sync_kernel<TILE_M256N64>()};

static int align4(int v) { return (v + 3) & ~3; }

static int g_cu_count = 0;
static int conv_cu_count() { return g_cu_count > 0 ? g_cu_count : 256; }

static int conv_geometry(const ConvArgs& a, int tile, bool pipe, ConvDev* d, ConvGeom* g) {
    if (tile < 0 || tile >= TILE_COUNT) return fail(FC_E_ARG, "conv: bad tile id");
    const TileInfo t = conv_tile_info(tile, pipe);
    if (!is_pow2(a.H) || !is_pow2(a.W)) return fail(FC_E_SHAPE, "conv: H and W must be powers of two");
    if ((a.s0.C & 3) || (a.s1.C & 3) || (a.Cout & 3)) return fail(FC_E_SHAPE, "conv: channel counts must be multiples of 4");
    if (a.s0.C + a.s1.C != a.Cin) return fail(FC_E_ARG, "conv: Cin != C0 + C1");
    if (a.stride != 1 && a.stride != 2) return fail(FC_E_SHAPE, "conv: stride must be 1 or 2");
    if (a.ups && a.stride != 1) return fail(FC_E_SHAPE, "conv: upsample needs stride 1");
    if (a.res_out && (a.s0.xf.mode || a.s1.xf.mode)) return fail(FC_E_ARG, "conv: fused res needs untransformed input");
    if (a.res_out && (a.pad >= a.KS)) return fail(FC_E_ARG, "conv: fused res needs a centre tap");
    if ((a.out_sh || a.pad_y >= 0 || a.pad_x >= 0) && (a.res_out || a.fin.gamma || a.stride != 1 || a.ups || a.out_sh > 1 || a.out_oy >> a.out_sh || a.out_ox >> a.out_sh))
        return fail(FC_E_ARG, "conv: the parity form (pad_y / pad_x / out_sh) is a plain stride-1 convolution");
    if (a.stats_tmul < 1 || a.stats_toff < 0 || a.stats_toff >= a.stats_tmul) return fail(FC_E_ARG, "conv: bad statistics slot");
    if (a.par4 && (a.KS != 2 || a.out_sh != 1 || a.stats_tmul != 4 || a.w_batch_stride || a.w4)) return fail(FC_E_ARG, "conv: par4 is the four-class form of a folded upsampling (2x2 taps, out_sh 1)");
    const int TW = a.W < 16 ? a.W : 16;
    int TH = t.BM / TW;
    if (TH > a.H) TH = a.H;
    const int TB = t.BM / (TH * TW);
    if (a.w_batch_stride && TB != 1) return fail(FC_E_SHAPE, "conv: per-sample weights need >= BM pixels per sample");
    ConvDev& p = *d;
    p.a = a;
    p.stamps = nullptr;
    p.TWl = ilog2(TW); p.THl = ilog2(TH); p.TB = TB;
    p.PH = TH * a.stride + a.KS - a.stride;
    p.PW = TW * a.stride + a.KS - a.stride;
    p.P = TB * p.PH * p.PW;
    p.magic_phw = p.PH * p.PW > 1 ? (unsigned)((1ull << 32) / (unsigned)(p.PH * p.PW)) + 1u : 0u;
    p.magic_pw = p.PW > 1 ? (unsigned)((1ull << 32) / (unsigned)p.PW) + 1u : 0u;
    p.tiles_x = a.W / TW; p.tiles_y = a.H / TH;
    p.ntiles = cdiv(a.Cout, t.BN);
    p.nblocks = cdiv(a.B, TB) * p.tiles_x * p.tiles_y * p.ntiles * (a.par4 ? 4 : 1);
    p.txl = ilog2(p.tiles_x); p.tyl = ilog2(p.tiles_y);
    p.magic_nt = (p.ntiles > 1 && p.nblocks < 65536) ? (unsigned)((1ull << 32) / (unsigned)p.ntiles) + 1u : 0u;   // exact for x < 2^16
    p.loader_prio = 0; p.o_epoch = p.o_gran = 0; p.o_out = -1; p.bf3 = 0;
    p.act0 = a.s0.xf.mode == 2; p.act1 = a.s1.xf.mode == 2;
    p.any_xf = (a.s0.xf.mode != 0) || (a.s1.xf.mode != 0);
    p.rps = TB > 1 ? a.H * a.W : t.BM;
    p.cpg = p.cpgt = p.NPG = 1;
    g->T = 0; g->n_t = 0.f;
    if (a.stats_out) {
        if (a.Gout <= 0 || a.Cout % a.Gout) return fail(FC_E_ARG, "conv: Cout not divisible by groups");
        if (p.rps % 16) return fail(FC_E_SHAPE, "conv: fused GroupNorm partials need >= 16 pixels per sample");
        p.cpg = a.Cout / a.Gout;
        if (!is_pow2(p.cpg)) return fail(FC_E_SHAPE, "conv: channels per group must be a power of two");
        p.cpgt = p.cpg < t.BN ? p.cpg : t.BN;
        p.NPG = p.cpg >= t.BN ? p.cpg / t.BN : 1;
        g->T = (TB > 1 ? 1 : p.tiles_x * p.tiles_y) * p.NPG;
        g->n_t = (float)(p.rps * p.cpgt);
    }
    g->pipe = pipe ? 1 : 0;
    if (pipe) {
        if (!conv_pipe_supports_ks(a.KS)) return fail(FC_E_SHAPE, "conv: kernel size not instantiated in the pipelined kernel");
        if (!conv_staging_fits(p.P, tile, a.KS, kPipeNPL)) return fail(FC_E_SHAPE, "conv: patch too large for the pipelined kernel");
        const int G0 = a.s0.xf.mode ? a.s0.xf.G : 0, G1 = a.s1.xf.mode ? a.s1.xf.G : 0;
        int o = 0;
        p.o_pixoff = p.o_pixtb = 0;
        p.o_epoch = o; o += 4;                     // fused tail: this launch's epoch, written in the prologue, read in the epilogue (never aliased)
        p.o_gstat = o; o += align4(2 * TB * (G0 + G1));
        p.o_aff = o; o += p.any_xf ? align4(2 * TB * a.Cin) : 0;
        p.o_patch = o;
        // M32N32K4 at 3x3 loads its weights global -> registers (conv_pipe.hip "DB"): no slab stages in LDS
        const bool direct_b = (t.WMWN == 1 && t.MTNT == 1 && a.KS == 3);
        // split-bf16 form (ConvArgs::prec): where an instantiation exists (conv_bf3_form), plain launches only (no fused res_conv / tail,
        // shared weights) whose weights exist pre-split (ConvArgs::w_b3, PACK_CONV_B3)
        p.bf3 = (a.prec == 1 && a.w_b3 && conv_bf3_form(tile, a.KS) && !a.res_out && !a.fin.gamma && !a.w_batch_stride) ? 1 : 0;
        p.patch_stride = align4(p.P * (t.CC + ((direct_b || p.bf3) ? 4 : 1)));    // (its k-step-quad form strides pixels by CC + 4 floats, and so does split-bf16)
        p.o_wl = o + 2 * p.patch_stride;
        p.wl_stride = direct_b ? 0 : a.KS * a.KS * t.CC * t.BN + (a.res_out ? t.CC * t.BN : 0);
        p.o_wres = 0;
        p.nchunks = cdiv(a.Cin, t.CC);
        // a third weight stage lets slabs run two chunks ahead of the MFMAs; only worth its LDS when there are chunks to run ahead of
        p.nwb = (p.nchunks >= 3 && (size_t)(o + 2 * p.patch_stride + 3 * p.wl_stride) * sizeof(float) <= 160 * 1024) ? 3 : 2;
        const int main_sz = 2 * p.patch_stride + p.nwb * p.wl_stride;
        int epi = 0;
        p.o_red = o;
        if (t.WK > 1) epi = t.WMWN * (t.WK - 1) * t.MTNT * (a.res_out ? 2 : 1) * 1024;
        p.o_part = o + epi;
        if (a.stats_out) epi += 2 * (t.BM / 16) * t.BN + 2 * TB * t.BN;
        p.o_fin = o + epi;
        if (a.fin.gamma) epi += 2 * TB * t.BN;
        p.o_gran = o + epi;
        if (a.fin.gamma) epi += align4(TB * (p.cpg >= t.BN ? 1 : t.BN / p.cpg) * g->T * 2);   // partials of every workgroup of the sample group, gathered
        p.o_out = -1;
        if ((size_t)(o + epi + t.BM * (t.BN + 4)) * sizeof(float) <= 160 * 1024) { p.o_out = o + epi; epi += t.BM * (t.BN + 4); }
        o += main_sz > epi ? main_sz : epi;
        p.zeros16 = conv_zeros16();
        p.stamps = conv_stamp_buffer();
        p.loader_prio = 1;   // measured: 1 = +1.5 %, 2 / 3 a little less (profiles/r02_*)
        g->tile = tile; g->grid = p.nblocks; g->lds = (size_t)o * sizeof(float);
        if (g->lds > 160 * 1024) return fail(FC_E_SHAPE, "conv: tile does not fit in LDS");
        p.gsz = 1; p.fin_local = 0;
        if (a.fin.gamma) {   // fused Block tail: shape conditions and, above all, residency of the whole grid
            if (!a.stats_out || a.stats_post || a.out_act || a.add || a.res_out) return fail(FC_E_ARG, "conv: fused tail excludes act / add / res outputs");
            if (a.Cout % t.BN && a.Cout > t.BN) return fail(FC_E_SHAPE, "conv: fused tail needs Cout to fill its column tiles");
            p.gsz = p.tiles_x * p.tiles_y * p.ntiles;
            g->groups = cdiv(a.B, TB);
            const int cpgt1 = a.Cout < t.BN ? a.Cout : t.BN, NPG1 = a.Cout >= t.BN ? a.Cout / t.BN : 1;
            g->T1 = (TB > 1 ? 1 : p.tiles_x * p.tiles_y) * NPG1;
            g->n_t1 = (float)(p.rps * cpgt1);
            p.fin_local = g->fin_local = (g->T == 1) ? 1 : 0;   // whole groups per tile: nothing to meet for
            if (p.fin_local) p.gsz = 1;
            g->gsz = p.gsz;
            if (!p.fin_local) {
                // Workgroups that wait for each other must all be resident.  How many of THIS instantiation one CU holds (registers,
                // waves, LDS) is asked of the runtime per flavour -- round 2 assumed "two when the LDS fits and NT = 1", an unverified
                // register-count claim -- and never counted above two.  This proves residency on a device the launch has to itself;
                // what keeps other work of this process away from it is the meeting guard in unet.hip, and a handle that shares the
                // device with anything else takes the plan without meetings (fc_unet_set_shared).
                int per_cu = conv_pipe_blocks_per_cu(p, tile, g->lds);
                if (per_cu <= 0) return fail(FC_E_SHAPE, "conv: fused tail: occupancy of the kernel unknown");
                if (per_cu > 2) per_cu = 2;
                if (p.nblocks > conv_cu_count() * per_cu) return fail(FC_E_SHAPE, "conv: fused tail needs the whole grid resident");
            }
        }
        return FC_OK;
    }
    if (a.fin.gamma) return fail(FC_E_SHAPE, "conv: fused tail is implemented in the pipelined kernel only");
    static_assert(kConvTiles[TILE_M256N64].CCs == 0, "the one tile without a synchronous form");
    if (tile == TILE_M256N64) return fail(FC_E_SHAPE, "conv: M256N64 exists in the pipelined kernel only");
    // LDS carve (in floats)
    int o = 0;
    p.o_pixoff = o; o += align4(p.P);
    p.o_pixtb = o; o += align4(p.P);
    const int G0 = a.s0.xf.mode ? a.s0.xf.G : 0, G1 = a.s1.xf.mode ? a.s1.xf.G : 0;
    p.o_gstat = o; o += align4(2 * TB * (G0 + G1));
    p.o_aff = o; o += align4(2 * TB * t.CC);
    p.o_patch = o;
    int main_sz = align4(p.P * (t.CC + 1));
    p.o_wl = o + main_sz; main_sz += a.KS * a.KS * t.CC * t.BN;
    p.o_wres = o + main_sz; if (a.res_out) main_sz += t.CC * t.BN;
    // epilogue scratch aliases patch/wl
    int epi = 0;
    p.o_red = o;
    if (t.WK > 1) epi = t.WMWN * (t.WK - 1) * t.MTNT * (a.res_out ? 2 : 1) * 1024;
    p.o_part = o + epi;
    if (a.stats_out) epi += 2 * (t.BM / 16) * t.BN + 2 * TB * t.BN;
    o += main_sz > epi ? main_sz : epi;
    g->tile = tile; g->grid = p.nblocks; g->lds = (size_t)o * sizeof(float);
    if (g->lds > 160 * 1024) return fail(FC_E_SHAPE, "conv: tile does not fit in LDS");
    return FC_OK;
}

bool conv_fin_possible(const ConvArgs& a, int tile) {
    ConvDev d;
    ConvGeom g;
    ConvArgs b = a;
    if (!b.fin.gamma) b.fin.gamma = reinterpret_cast<const float*>(16);   // geometry only
    if (!b.stats_out) b.stats_out = reinterpret_cast<float*>(16);
    return conv_geometry(b, tile, true, &d, &g) == FC_OK;   // a refusal leaves its reason in fc_last_error, harmlessly
}

// The launch (a Block-closing one the plan has accepted: every pointer real) is the one the step-closing flavour is compiled for, and
// that flavour -- its own registers and LDS, asked of the runtime like every meeting launch's -- keeps the whole grid resident too.
bool conv_step_close_possible(const ConvArgs& a, int tile) {
    static StepClose dummy;
    ConvDev d;
    ConvGeom g;
    if (!a.fin.gamma || conv_geometry(a, tile, true, &d, &g) != FC_OK || !conv_pipe_step_ok(d, tile)) return false;
    d.a.fin.step = &dummy;      // (never dereferenced: the occupancy query launches nothing)
    d.stamps = nullptr;
    int per_cu = conv_pipe_blocks_per_cu(d, tile, g.lds);
    if (per_cu > 2) per_cu = 2;
    return per_cu > 0 && d.nblocks <= conv_cu_count() * per_cu;
}

static int auto_tile(const ConvArgs& a) {
    const long M = (long)a.B * a.H * a.W;
    const int hw = a.H * a.W;
    auto T = [](int t) { return conv_tile_info(t, true); };      // (BM and BN are those of both kernels)
    auto blocks = [&](int t) { return (M / T(t).BM) * cdiv(a.Cout, T(t).BN) * (a.par4 ? 4 : 1); };   // (par4: four classes per launch)
    auto ok = [&](int t) { return !(a.w_batch_stride && hw < T(t).BM) && M >= T(t).BM; };
    // Data gradients of the 256-channel 3x3 layers at 4x4 (unet_backward.hip dgrad_to): at 256 rows the thresholds below give them M128N32,
    // ONE accumulation chain over K = 2304, whose rounding (7.4e-7 of the result on random data, against 2.7e-7 for four chains of 576)
    // is past what the backward's pass-through gate allows; the four-chain tile is also the faster one there (256 -> 256: 52.6 against
    // 62 us, 256 -> 128: 27.4 against 60.6 us, back to back at B = 256)
    if (a.split_long_k && hw <= 16 && (long)a.Cin * a.KS * a.KS >= 2048 && ok(TILE_M32N32K4)) return TILE_M32N32K4;
    // measured on the SD-VAE shapes (tools/conv_microbench.py --vae, B=16): M256N64 113 / 109 / 101 TFLOP/s at 512@64^2 / 256@128^2 /
    // 128@256^2 against 101 / 97 / 90 for M128N64 and 98 / 105 / 98 for M128N32; the 64-wide column tile only pays for 1x1 layers
    if (a.Cout >= 64 && ok(TILE_M256N64) && blocks(TILE_M256N64) >= 512) {
        ConvDev d;
        ConvGeom g;
        if (conv_geometry(a, TILE_M256N64, true, &d, &g) == FC_OK) return TILE_M256N64;   // else: patch / LDS limits, fall through
    }
    if (a.par4) {   // four 2x2-tap classes in one launch: a workgroup has 4/9 of a 3x3 layer's matrix work, so the grid wants to be twice as full
                    // before a larger tile pays (measured at B = 64: 128->64 @8->16 M32N32K4 18.7 against M128N32 21.7 us; 64->32 @16->32 M128N32 14.6 against M64N32K2 18.3)
        if (ok(TILE_M128N32) && blocks(TILE_M128N32) >= 512) return TILE_M128N32;
        if (ok(TILE_M64N32K2) && blocks(TILE_M64N32K2) >= 512) return TILE_M64N32K2;
        return TILE_M32N32K4;
    }
    if ((a.KS == 1 || a.Cout >= 512) && a.Cout >= 64 && ok(TILE_M128N64) && blocks(TILE_M128N64) >= 512) return TILE_M128N64;
    if (ok(TILE_M128N32) && blocks(TILE_M128N32) >= 256) return TILE_M128N32;   // one full wave of workgroups: measured 20 vs 29 us on the 64-channel 16x16 layers (profiles/r01_c_conv_microbench.txt)
    if (a.Cout >= 64 && ok(TILE_M64N64K2) && blocks(TILE_M64N64K2) >= 384) return TILE_M64N64K2;
    if (ok(TILE_M64N32K2) && blocks(TILE_M64N32K2) >= 256) return TILE_M64N32K2;
    return TILE_M32N32K4;
}

static unsigned long long* g_stamps = nullptr;
unsigned long long* conv_stamp_buffer() { return g_stamps; }
void conv_set_stamp_buffer(unsigned long long* p) { g_stamps = p; }

// pipelined kernel when its constraints hold, else the synchronous one
static int geometry_best(const ConvArgs& a, int tile, ConvDev* d, ConvGeom* g) {
    if (conv_geometry(a, tile, true, d, g) == FC_OK) return FC_OK;
    return conv_geometry(a, tile, false, d, g);
}

int conv_plan(const ConvArgs& a, int tile, ConvGeom* g) {
    ConvDev d;
    if (tile == TILE_AUTO) tile = auto_tile(a);
    return geometry_best(a, tile, &d, g);
}

// Once per process, before any launch or graph capture: let every instantiation use the full 160 KiB of LDS.
int conv_init() {
    static bool done = false;
    if (done) return FC_OK;
    for (SyncKernel k : kSyncKernels)
        if (k) FC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    FC_TRY(conv_pipe_init());
    {
        int dev = 0;
        hipDeviceProp_t prop;
        FC_HIP(hipGetDevice(&dev));
        FC_HIP(hipGetDeviceProperties(&prop, dev));
        g_cu_count = prop.multiProcessorCount;
    }
    done = true;
    return FC_OK;
}

int conv_launch(const ConvArgs& a, int tile, hipStream_t s) {
    ConvDev d;
    ConvGeom g;
    if (tile == TILE_AUTO) tile = auto_tile(a);
    FC_TRY(geometry_best(a, tile, &d, &g));
    if (g.pipe) return conv_pipe_launch(d, tile, g.grid, g.lds, s);
    if (!kSyncKernels[tile]) return fail(FC_E_ARG, "conv: bad tile id");
    hipLaunchKernelGGL(kSyncKernels[tile], dim3(g.grid), dim3(256), g.lds, s, d);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

}  // namespace fc
