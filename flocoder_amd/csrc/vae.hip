// Native runtime of the SD-VAE codec (flocoder's SD_VAE_Wrapper, codecs.py:631-663 -> diffusers AutoencoderKL): parameter
// table with the upstream state_dict names, weight packing, and one launch plan each for encode and decode.
//
// The architecture is third-party (diffusers is not part of the reference tree; parity unpinned -- DESIGN.md 2).  Every
// Conv2d runs on the implicit-GEMM kernel; the pre-norm resnets map onto it directly:
//     norm1 -> SiLU -> conv1      = conv with GroupNorm(32, eps 1e-6)+SiLU applied by the loader to the raw input
//     norm2 -> SiLU -> conv2 (+x) = the same, with the shortcut added in the epilogue and the statistics for the NEXT
//                                   block's norm1 taken from the final sum (ConvArgs::stats_post)
// so no normalised / activated tensor is ever materialised.  Downsample2D's pad(0,1,0,1)+conv3x3/s2 is a stride-2 launch
// with pad 0 (reads beyond the bottom/right edge are the loader's zero fill); Upsample2D's nearest x2 is folded into the
// following conv's loader.  The single-head mid-block attention (n = h*w tokens, d = 512) is three 1x1 convs, a batched
// transpose, two per-sample-weight GEMMs on the same kernel (scores = q k^T, out = softmax v) and a one-pass row softmax.
#include <cstring>
#include <memory>

#include "codec.h"

using namespace fc;

struct fc_vae : fc::Codec {
    int in_ch = 3, latent = 4, lpb = 2, groups = 32;
    std::vector<int> bo{128, 256, 512, 512};
};

namespace fc {

static constexpr float kEps = 1e-6f;

static void decl_resnet(fc_vae* v, const std::string& n, int ci, int co) {
    v->decl_norm(n + ".norm1", ci);
    v->decl_conv(n + ".conv1", co, ci, 3);
    v->decl_norm(n + ".norm2", co);
    v->decl_conv(n + ".conv2", co, co, 3);
    if (ci != co) v->decl_conv(n + ".conv_shortcut", co, ci, 1);
}
static void decl_mid(fc_vae* v, const std::string& n, int c) {
    decl_resnet(v, n + ".resnets.0", c, c);
    const std::string a = n + ".attentions.0";
    v->decl_norm(a + ".group_norm", c);
    v->decl_linear_t(a + ".to_q", c, c);
    v->decl_linear_t(a + ".to_k", c, c);
    v->decl_linear_t(a + ".to_v", c, c);
    v->decl_linear_t(a + ".to_out.0", c, c);
    decl_resnet(v, n + ".resnets.1", c, c);
}
static int declare_all(fc_vae* v) {
    const std::vector<int>& bo = v->bo;
    const int L = (int)bo.size();
    v->decl_conv_pad("encoder.conv_in", bo[0], v->in_ch, 3, bo[0], 4, false);      // RGB in / out: channels zero-padded to 4
    int ci = bo[0];
    for (int i = 0; i < L; ++i) {
        for (int j = 0; j < v->lpb; ++j) decl_resnet(v, "encoder.down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), j == 0 ? ci : bo[i], bo[i]);
        if (i < L - 1) v->decl_conv("encoder.down_blocks." + std::to_string(i) + ".downsamplers.0.conv", bo[i], bo[i], 3);
        ci = bo[i];
    }
    decl_mid(v, "encoder.mid_block", bo[L - 1]);
    v->decl_norm("encoder.conv_norm_out", bo[L - 1]);
    v->decl_conv("encoder.conv_out", 2 * v->latent, bo[L - 1], 3);
    v->decl_conv("quant_conv", 2 * v->latent, 2 * v->latent, 1);
    v->decl_conv("post_quant_conv", v->latent, v->latent, 1);
    v->decl_conv("decoder.conv_in", bo[L - 1], v->latent, 3);
    decl_mid(v, "decoder.mid_block", bo[L - 1]);
    ci = bo[L - 1];
    for (int i = 0; i < L; ++i) {
        const int co = bo[L - 1 - i];
        for (int j = 0; j < v->lpb + 1; ++j) decl_resnet(v, "decoder.up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), j == 0 ? ci : co, co);
        if (i < L - 1) v->decl_conv_up2("decoder.up_blocks." + std::to_string(i) + ".upsamplers.0.conv", co, co);
        ci = co;
    }
    v->decl_norm("decoder.conv_norm_out", bo[0]);
    v->decl_conv_pad("decoder.conv_out", v->in_ch, bo[0], 3, 4, bo[0], true);
    return FC_OK;
}

struct VBuilder : PlanBuilder {
    fc_vae* v;
    VBuilder(fc_vae* v_, Plan* pl_, int B_) : v(v_) { pl = pl_; B = B_; store = v_; }

    SrcXform gn(const Stat& st, const std::string& norm, int mode) { return xf_of(st, mode, v->R(norm + ".weight"), v->R(norm + ".bias"), nullptr, 0, kEps); }

    // x (+ its GroupNorm(32) partials) -> resnet output (+ partials when the consumer starts with a norm)
    // The pre-norm input of each convolution is a tensor of its own (PlanBuilder::activated).  Round 3: one elementwise launch writes
    // act(GN(x)) and the convolution reads that.  Rounds 1-2 normalised in the convolution's staging waves and never materialised the
    // tensor, which saves one round trip through HBM but transforms every window element once per output-channel tile and halo copy --
    // ~10x at 512 channels -- and VALU work of the staging waves does not overlap the MFMAs of the waves they share a SIMD with
    // (DESIGN.md 5): measured per resnet, fp32: 1.40 -> 1.29 + 0.03 ms at 512 channels, 6.32 -> 5.79 + 0.43 ms at 128; split-bf16:
    // 0.55 -> 0.45 + 0.03, 2.89 -> 2.38 + 0.43.
    Act resnet(const std::string& n, const Act& x, const Stat& sx, int co, bool want_stats, Stat* so) {
        scope = n;
        const int G = v->groups;
        Act h1 = act(co, x.H, x.W);
        Stat s1;
        Act t1 = activated(x, gn(sx, n + ".norm1", 2));
        conv(layer(n + ".conv1", t1, 3), h1, G, &s1);
        release(t1);
        Act sc = x;
        const bool proj = x.C != co;
        if (proj) {
            sc = act(co, x.H, x.W);
            conv(layer(n + ".conv_shortcut", x, 1), sc, 0, nullptr);
        }
        Act out = act(co, x.H, x.W);
        Act t2 = activated(h1, gn(s1, n + ".norm2", 2));
        ConvArgs b = layer(n + ".conv2", t2, 3);
        b.add = sc.p; b.stats_post = 1;
        conv(b, out, want_stats ? G : 0, so);
        release(t2);
        tap(n, out); tap(n + ".h1", h1);
        release(h1);
        if (proj) release(sc);
        return out;
    }

    // mid-block attention: out = to_out(softmax(q k^T / sqrt(C)) v) + x, q/k/v = Linear(GroupNorm(x))
    Act attention(const std::string& n, const Act& x, const Stat& sx, Stat* so) {
        scope = n;
        Act out = attention_block(x, gn(sx, n + ".group_norm", 1), {n + ".to_q", n + ".to_k", n + ".to_v", n + ".to_out.0"}, v->groups, so);
        tap(n, out);
        return out;
    }

    Act mid(const std::string& n, Act x, Stat sx, Stat* so) {
        Stat s1, s2;
        Act a = resnet(n + ".resnets.0", x, sx, x.C, true, &s1);
        release(x);
        Act b = attention(n + ".attentions.0", a, s1, &s2);
        release(a);
        Act c = resnet(n + ".resnets.1", b, s2, x.C, true, so);
        release(b);
        return c;
    }
};

static int build_encoder(fc_vae* v, int maxB, int H, int W) {
    v->enc.release();
    const int L = (int)v->bo.size();
    if (!is_pow2(H) || !is_pow2(W) || (H >> (L - 1)) < 1 || (W >> (L - 1)) < 1) return fail(FC_E_SHAPE, "vae: image height/width must be powers of two >= 8");
    VBuilder b(v, &v->enc, maxB);
    b.conv_prec = v->prec; b.keep_all = v->taps != 0;
    const int G = v->groups, ic = v->in_ch;
    Act xin = b.act(4, H, W);
    float* xp = xin.p;
    b.scope = "input";
    b.push([=](const FwdCtx& c, hipStream_t s) { return nchw_to_nhwc_launch(c.x, xp, c.B, ic, H * W, 4, c.B, s); }, "nchw_to_nhwc");
    Stat st;
    Act x = b.act(v->bo[0], H, W);
    {
        b.scope = "encoder.conv_in";
        b.conv(b.layer(b.scope, xin, 3), x, G, &st);
        b.tap(b.scope, x);
    }
    for (int i = 0; i < L && !b.err; ++i) {
        const std::string blk = "encoder.down_blocks." + std::to_string(i);
        for (int j = 0; j < v->lpb && !b.err; ++j) {
            const bool last = j == v->lpb - 1, down = i < L - 1;
            Stat so;
            Act y = b.resnet(blk + ".resnets." + std::to_string(j), x, st, v->bo[i], !(last && down), &so);
            b.release(x);
            x = y; st = so;
        }
        if (i < L - 1 && !b.err) {   // Downsample2D: pad (0,1,0,1) + conv3x3 stride 2
            b.scope = blk + ".downsamplers.0";
            Act y = b.act(v->bo[i], x.H / 2, x.W / 2);
            ConvArgs a = b.layer(blk + ".downsamplers.0.conv", x, 3);
            a.pad = 0; a.stride = 2;
            b.conv(a, y, G, &st);
            b.tap(b.scope, y);
            b.release(x);
            x = y;
        }
    }
    if (b.err) return b.err;
    Stat sm;
    x = b.mid("encoder.mid_block", x, st, &sm);
    if (b.err) return b.err;
    Act mo = b.act(2 * v->latent, x.H, x.W), qo = b.act(2 * v->latent, x.H, x.W);
    {
        b.scope = "encoder.conv_out";
        ConvArgs a = b.layer(b.scope, x, 3);
        a.s0.xf = b.gn(sm, "encoder.conv_norm_out", 2);
        b.conv(a, mo, 0, nullptr);
        b.tap(b.scope, mo);
        b.scope = "quant_conv";
        b.conv(b.layer(b.scope, mo, 1), qo, 0, nullptr);
        b.tap(b.scope, qo);
    }
    if (b.err) return b.err;
    const float* qp = qo.p;
    const int lat = v->latent, hw = x.H * x.W;
    b.scope = "latent_dist.mean";
    b.push([=](const FwdCtx& c, hipStream_t s) { return nhwc_to_nchw_launch(qp, c.out, c.B, lat, hw, 2 * lat, s); }, "nhwc_to_nchw");
    v->enc.maxB = maxB; v->enc.H = H; v->enc.W = W;
    return FC_OK;
}

static int build_decoder(fc_vae* v, int maxB, int h, int w) {
    v->dec.release();
    const int L = (int)v->bo.size();
    if (!is_pow2(h) || !is_pow2(w)) return fail(FC_E_SHAPE, "vae: latent height/width must be powers of two");
    VBuilder b(v, &v->dec, maxB);
    b.conv_prec = v->prec; b.keep_all = v->taps != 0;
    const int G = v->groups, lat = v->latent, top = v->bo[L - 1];
    Act zin = b.act(lat, h, w), z1 = b.act(lat, h, w);
    float* zp = zin.p;
    b.scope = "input";
    b.push([=](const FwdCtx& c, hipStream_t s) { return nchw_to_nhwc_launch(c.x, zp, c.B, lat, h * w, lat, c.B, s); }, "nchw_to_nhwc");
    Stat st;
    Act x = b.act(top, h, w);
    {
        b.scope = "post_quant_conv";
        b.conv(b.layer(b.scope, zin, 1), z1, 0, nullptr);
        b.tap(b.scope, z1);
        b.scope = "decoder.conv_in";
        b.conv(b.layer(b.scope, z1, 3), x, G, &st);
        b.tap(b.scope, x);
    }
    if (b.err) return b.err;
    Stat sm;
    x = b.mid("decoder.mid_block", x, st, &sm);
    st = sm;
    for (int i = 0; i < L && !b.err; ++i) {
        const std::string blk = "decoder.up_blocks." + std::to_string(i);
        const int co = v->bo[L - 1 - i];
        for (int j = 0; j < v->lpb + 1 && !b.err; ++j) {
            const bool last = j == v->lpb, up = i < L - 1;
            Stat so;
            Act y = b.resnet(blk + ".resnets." + std::to_string(j), x, st, co, !(last && up), &so);
            b.release(x);
            x = y; st = so;
        }
        if (i < L - 1 && !b.err) {   // Upsample2D: nearest x2 + conv3x3
            b.scope = blk + ".upsamplers.0";
            Act y = b.act(co, x.H * 2, x.W * 2);
            // (round 3) the upsampling is folded into the weights: four 2x2 convolutions on x, 4/9 of the multiply-adds (plan.h conv_up2);
            // FLOCODER_AMD_UPS_FOLD=0: the 3x3 convolution over the upsampled window as in rounds 1-2
            ConvArgs a = b.layer(blk + ".upsamplers.0.conv", x, 3);
            a.ups = 1;
            if (!b.conv_up2(x, v->PUP(blk + ".upsamplers.0.conv.weight"), a.bias, y, G, &st)) b.conv(a, y, G, &st);
            b.tap(b.scope, y);
            b.release(x);
            x = y;
        }
    }
    if (b.err) return b.err;
    Act yo = b.act(4, x.H, x.W);
    {
        b.scope = "decoder.conv_out";
        ConvArgs a = b.layer(b.scope, x, 3);            // (its bias is the packed, zero-padded one: ParamStore::bias)
        a.s0.xf = b.gn(st, "decoder.conv_norm_out", 2);
        b.conv(a, yo, 0, nullptr);
        b.tap(b.scope, yo);
    }
    if (b.err) return b.err;
    const float* yp = yo.p;
    const int ic = v->in_ch, HW = x.H * x.W;
    b.scope = "sample";
    b.push([=](const FwdCtx& c, hipStream_t s) { return nhwc_to_nchw_launch(yp, c.out, c.B, ic, HW, 4, s); }, "nhwc_to_nchw");
    v->dec.maxB = maxB; v->dec.H = h; v->dec.W = w;
    return FC_OK;
}

}  // namespace fc

extern "C" {

int fc_vae_create(int device, fc_vae** out) {
    if (!out) return fail(FC_E_ARG, "fc_vae_create: null argument");
    return codec_create(std::unique_ptr<fc_vae>(new fc_vae), device, declare_all, out);
}
void fc_vae_destroy(fc_vae* v) { codec_destroy(v); }

int fc_vae_param_count(const fc_vae* v) { return v ? (int)v->params.size() : 0; }
int64_t fc_vae_param_numel(const fc_vae* v) { return v ? v->raw_numel : 0; }
int fc_vae_param_info(const fc_vae* v, int i, const char** name, int64_t shape[4], int64_t* offset) {
    if (!v) return fail(FC_E_ARG, "fc_vae_param_info: null handle");
    return v->info(i, name, shape, offset);
}
int fc_vae_load_params(fc_vae* v, const float* flat, int64_t numel, int on_device, void* stream) {
    return codec_load(v, "fc_vae_load_params", flat, numel, on_device, stream);
}
int fc_vae_set_precision(fc_vae* v, int mode) { return codec_set_precision(v, "fc_vae_set_precision", mode); }
int fc_vae_debug_taps(fc_vae* v, int on) { return codec_debug_taps(v, "fc_vae_debug_taps", on); }
int fc_vae_debug_tensor(const fc_vae* v, int decode, const char* name, const float** ptr, int* C, int* H, int* W) {
    return codec_debug_tensor(v, "fc_vae_debug_tensor", decode, name, ptr, C, H, W);
}
int fc_vae_reserve_encode(fc_vae* v, int max_batch, int height, int width) {
    return codec_reserve(v, "fc_vae_reserve_encode", 0, build_encoder, max_batch, height, width);
}
int fc_vae_reserve_decode(fc_vae* v, int max_batch, int lat_height, int lat_width) {
    return codec_reserve(v, "fc_vae_reserve_decode", 1, build_decoder, max_batch, lat_height, lat_width);
}
int fc_vae_encode(fc_vae* v, const float* x_dev, float* mean_out_dev, int batch, int height, int width, void* stream) {
    return codec_run(v, "fc_vae_encode", 0, x_dev, mean_out_dev, batch, height, width, stream);
}
int fc_vae_decode(fc_vae* v, const float* z_dev, float* x_out_dev, int batch, int lat_height, int lat_width, void* stream) {
    return codec_run(v, "fc_vae_decode", 1, z_dev, x_out_dev, batch, lat_height, lat_width, stream);
}
double fc_vae_flops_per_sample(const fc_vae* v, int decode) { return v ? v->plan(decode).flops : 0.0; }
int fc_vae_plan_launches(const fc_vae* v, int decode) { return v ? (int)v->plan(decode).ops.size() : 0; }
int fc_vae_op_info(const fc_vae* v, int decode, int i, const char** kernel, const char** module, double* flops_per_sample) {
    return codec_op_info(v, "fc_vae_op_info", decode, i, kernel, module, flops_per_sample, nullptr, nullptr);
}
int fc_vae_op_bytes(const fc_vae* v, int decode, int i, double* bytes_per_sample, double* bytes_per_launch) {
    return codec_op_info(v, "fc_vae_op_bytes", decode, i, nullptr, nullptr, nullptr, bytes_per_sample, bytes_per_launch);
}
int fc_vae_profile_ops(fc_vae* v, int decode, const float* in_dev, float* out_dev, int batch, int repeats, float* ms_out, int n_out, void* stream) {
    return codec_profile(v, "fc_vae_profile_ops", decode, in_dev, out_dev, batch, repeats, ms_out, n_out, stream);
}

}  // extern "C"
