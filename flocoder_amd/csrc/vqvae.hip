// Native runtime of flocoder's VQVAE codec, encode / decode path (codecs.py:150-574; NATTEN-less, eval): parameter table with
// the reference's state_dict names and one launch plan each for VQVAE.encode (= self.encoder) and VQVAE.decode (= self.decoder at
// noise_strength 0).  quantize() (ResidualVQ, third-party) is not built.
//
// EncDecResidualBlock is post-norm:  out = SiLU(GN(conv2(SiLU(GN(conv1 x)))) + identity),  identity = x or GN(conv1x1/s x).
// On the implicit-GEMM kernel that is: conv1 (+ partials) | one finalize pass that writes SiLU(GN(.)) | conv2 (+ partials) | optional
// 1x1 projection (+ partials) | one finalize pass that normalises both branches, adds and applies SiLU.  Upsampling is
// conv3x3 -> SiLU (epilogue) -> PixelShuffle(2) (one re-layout pass).
#include <memory>

#include "codec.h"

using namespace fc;

struct fc_vqvae_config_s { int in_channels, hidden_channels, num_downsamples, internal_dim, vq_embedding_dim, decoder_nonlocal, natten = 0; };

struct fc_vqvae : fc::Codec {
    fc_vqvae_config_s c{3, 256, 3, 256, 4, 1, 0};
};

namespace fc {

static int gn_groups(int proposed, int channels) {   // codecs.py:34-44
    if (channels % proposed == 0) return proposed;
    for (int c = proposed; c < channels; ++c) if (channels % c == 0) return c;
    return 1;
}
static int pad4(int c) { return (c + 3) & ~3; }

// Conv2d with channel counts that are not multiples of 4 (pixel-space ends): zero-padded operands
static void decl_conv_any(fc_vqvae* v, const std::string& n, int O, int I, int K) {
    if (pad4(O) == O && pad4(I) == I) v->decl_conv(n, O, I, K);
    else v->decl_conv_pad(n, O, I, K, pad4(O), pad4(I), true);
}

// attn: 0 none | 1 AttnBlock ('full', codecs.py:52-90) | 2 NATTENBlock ('natten', codecs.py:93-145: GroupNorm, bias-free qkv / proj Linears, scalar gate)
static void decl_block(fc_vqvae* v, const std::string& n, int ci, int co, int stride, int attn) {
    const bool full_attn = attn == 1;
    decl_conv_any(v, n + ".conv1", co, ci, 3);
    v->decl_norm(n + ".norm1", co);
    v->decl_conv(n + ".conv2", co, co, 3);
    v->decl_norm(n + ".norm2", co);
    if (stride != 1 || ci != co) { decl_conv_any(v, n + ".downsample.0", co, ci, 1); v->decl_norm(n + ".downsample.1", co); }
    if (full_attn) {
        v->decl_norm(n + ".attn.norm.norm", co);
        for (const char* p : {".attn.q", ".attn.k", ".attn.v", ".attn.proj_out"}) v->decl_conv(n + p, co, co, 1);
    }
    if (attn == 2) {   // state_dict order of NATTENBlock: its own parameter (gamma) first, then the sub-modules norm, qkv, proj
        v->declare(n + ".attn.gamma", {1});
        v->decl_norm(n + ".attn.norm", co);
        v->decl_linear_t(n + ".attn.qkv", 3 * co, co, false);   // nn.Linear [out][in] -> operand [in][out]
        v->decl_linear_t(n + ".attn.proj", co, co, false);
    }
}

static int declare_all(fc_vqvae* v) {
    const auto& c = v->c;
    const int nd = c.num_downsamples, hid = c.hidden_channels, emb = c.vq_embedding_dim;
    int cur = c.in_channels;
    const int na = c.natten ? 2 : 0;       // with NATTEN: the last two encoder levels and the bottleneck block (codecs.py:414-429)
    for (int i = 0; i < nd; ++i) {
        const int co = hid << i, at = i >= nd - 2 ? na : 0;
        decl_block(v, "encoder." + std::to_string(2 * i), cur, co, 2, at);
        decl_block(v, "encoder." + std::to_string(2 * i + 1), co, co, 1, at);
        cur = co;
    }
    decl_block(v, "encoder." + std::to_string(2 * nd), cur, c.internal_dim, 1, na);
    v->decl_conv("encoder." + std::to_string(2 * nd + 1), c.internal_dim, c.internal_dim, 1);
    v->decl_conv("encoder." + std::to_string(2 * nd + 2), emb, c.internal_dim, 1);
    v->decl_norm("encoder." + std::to_string(2 * nd + 3), emb);
    v->decl_conv("encoder." + std::to_string(2 * nd + 5), emb, emb, 3);
    // decoder (codecs.py:245-316)
    const std::string L = "decoder.layers.";
    int i = 0;
    if (c.decoder_nonlocal) {
        const int cr = emb / 2 > 1 ? emb / 2 : 1;
        v->declare(L + "0.q_proj.weight", {cr, emb, 1, 1}); v->declare(L + "0.q_proj.bias", {cr});
        v->declare(L + "0.k_proj.weight", {cr, emb, 1, 1}); v->declare(L + "0.k_proj.bias", {cr});
        v->declare(L + "0.v_proj.weight", {emb, emb, 1, 1}); v->declare(L + "0.v_proj.bias", {emb});
        v->declare(L + "0.out_proj.weight", {emb, emb, 1, 1}); v->declare(L + "0.out_proj.bias", {emb});
        i = 1;
    }
    cur = hid << (nd - 1);
    v->decl_conv(L + std::to_string(i), c.internal_dim, emb, 1);
    v->decl_norm(L + std::to_string(i + 1), c.internal_dim);
    v->decl_conv(L + std::to_string(i + 3), cur, c.internal_dim, 1);
    decl_block(v, L + std::to_string(i + 5), cur, cur, 1, c.decoder_nonlocal ? 1 : na);   // attn = 'full' if decoder_nonlocal else 'natten' (codecs.py:266)
    i += 6;
    for (int lvl = nd - 1; lvl >= 0; --lvl) {
        int co = hid << (lvl - 1 > 0 ? lvl - 1 : 0);
        if (lvl == 0) co = hid;
        v->decl_conv(L + std::to_string(i), 4 * cur, cur, 3);
        decl_block(v, L + std::to_string(i + 4), cur, co, 1, lvl > nd - 2 ? na : 0);                // first upsampling level only (codecs.py:275-278)
        decl_block(v, L + std::to_string(i + 6), co, co, 1, 0);
        cur = co;
        i += 7;
    }
    v->decl_conv(L + std::to_string(i + 1), 64, cur, 3);
    decl_conv_any(v, L + std::to_string(i + 4), c.in_channels, 64, 3);
    return FC_OK;
}

struct QBuilder : PlanBuilder {
    fc_vqvae* v;
    QBuilder(fc_vqvae* v_, Plan* pl_, int B_) : v(v_) { pl = pl_; B = B_; store = v_; }

    SrcXform gn(const Stat& st, const std::string& norm, int mode, float eps = 1e-5f) {
        return xf_of(st, mode, v->R(norm + ".weight"), v->R(norm + ".bias"), nullptr, 0, eps);
    }

    // EncDecResidualBlock (codecs.py:150-214).  x is a raw NHWC tensor with x.C possibly padded to 4 (pixel input).
    Act block(const std::string& n, const Act& x, int co, int stride) {
        scope = n;
        const int G = gn_groups(8, co), Ho = x.H / stride, Wo = x.W / stride;
        Act h1 = act(co, Ho, Wo);
        Stat s1, s2, sd;
        ConvArgs a = layer(n + ".conv1", x, 3);
        a.stride = stride;
        conv(a, h1, G, &s1);
        // (round 3) conv2, or the attention in front of it, reads the activated tensor from memory instead of normalising it in its staging
        // waves once per output-channel tile and halo copy (vae.hip VBuilder::resnet has the measurements)
        const Act a1 = activated(h1, gn(s1, n + ".norm1", 2));
        Act mid_in = a1;
        if (v->has(n + ".attn.q.weight")) {                       // attention='full': AttnBlock on the activated tensor (codecs.py:190-192)
            const Stat sa = gn_stats(a1, gn_groups(32, co));
            mid_in = attention_block(a1, gn(sa, n + ".attn.norm.norm", 1, 1e-6f),
                                     {n + ".attn.q", n + ".attn.k", n + ".attn.v", n + ".attn.proj_out"}, 0, nullptr);
            tap(n + ".act", a1);
            release(a1);
        }
        if (v->has(n + ".attn.qkv.weight")) {                     // attention='natten': NATTENBlock on the activated tensor (codecs.py:93-145)
            const Stat sa = gn_stats(a1, gn_groups(8, co));
            Act qkv = act(3 * co, Ho, Wo), att = act(co, Ho, Wo), a2 = act(co, Ho, Wo);
            ConvArgs q = layer(n + ".attn.qkv", a1, 1);
            q.s0.xf = gn(sa, n + ".attn.norm", 1);
            conv(q, qkv, 0, nullptr);
            const float *qp = qkv.p, *gam = v->R(n + ".attn.gamma");
            float* tp = att.p;
            const int mode = v->c.natten;
            push([=](const FwdCtx& c, hipStream_t s) { return na2d_launch(qp, tp, gam, c.B, Ho, Wo, co, 8, 7, mode, s); }, "na2d",
                 2.0 * 2 * 49 * (double)co * Ho * Wo);
            ConvArgs pj = layer(n + ".attn.proj", att, 1);          // identity + gamma * proj(att): gamma rides in na2d's output (proj is linear, no bias)
            pj.add = a1.p;
            conv(pj, a2, 0, nullptr);
            tap(n + ".act", a1); tap(n + ".qkv", qkv); tap(n + ".att", att);    // .att carries gamma
            release(qkv); release(att); release(a1);
            mid_in = a2;
        }
        Act h2 = act(co, Ho, Wo);
        conv(layer(n + ".conv2", mid_in, 3), h2, G, &s2);
        tap(n + ".h1", h1); tap(n + ".mid", mid_in); tap(n + ".h2", h2);
        release(mid_in);
        Act out = act(co, Ho, Wo);
        FinalizeArgs f = fin_of(h2, gn(s2, n + ".norm2", 1), out);
        f.act_after_add = 1;
        Act d;
        if (v->has(n + ".downsample.0.weight")) {
            d = act(co, Ho, Wo);
            ConvArgs c = layer(n + ".downsample.0", x, 1);
            c.stride = stride;
            conv(c, d, G, &sd);
            f.res = d.p; f.xf_res = gn(sd, n + ".downsample.1", 1);
        } else {
            f.res = x.p;
        }
        finalize(f);
        tap(n, out);
        if (d.p) tap(n + ".res", d);
        release(h1); release(h2);
        if (d.p) release(d);
        return out;
    }
};

static int build_encoder(fc_vqvae* v, int maxB, int H, int W) {
    v->enc.release();
    const auto& c = v->c;
    const int nd = c.num_downsamples, emb = c.vq_embedding_dim;
    if (!is_pow2(H) || !is_pow2(W) || (H >> nd) < 4 || (W >> nd) < 4) return fail(FC_E_SHAPE, "vqvae: image size must be a power of two, >= 4 latent pixels per side");
    QBuilder b(v, &v->enc, maxB);
    b.conv_prec = v->prec; b.keep_all = v->taps != 0;
    const int ic = c.in_channels, icp = pad4(ic);
    Act x = b.act(icp, H, W);
    float* xp = x.p;
    b.scope = "input";
    b.push([=](const FwdCtx& cx, hipStream_t s) { return nchw_to_nhwc_launch(cx.x, xp, cx.B, ic, H * W, icp, cx.B, s); }, "nchw_to_nhwc");
    for (int i = 0; i < nd && !b.err; ++i) {
        Act y = b.block("encoder." + std::to_string(2 * i), x, c.hidden_channels << i, 2);
        b.release(x);
        Act z = b.block("encoder." + std::to_string(2 * i + 1), y, c.hidden_channels << i, 1);
        b.release(y);
        x = z;
    }
    if (b.err) return b.err;
    Act y = b.block("encoder." + std::to_string(2 * nd), x, c.internal_dim, 1);
    b.release(x);
    if (b.err) return b.err;
    Act t1 = b.act(c.internal_dim, y.H, y.W), t2 = b.act(emb, y.H, y.W), t3 = b.act(emb, y.H, y.W);
    Stat st;
    {
        b.scope = "encoder.compress";
        b.conv(b.layer("encoder." + std::to_string(2 * nd + 1), y, 1), t1, 0, nullptr);
        b.conv(b.layer("encoder." + std::to_string(2 * nd + 2), t1, 1), t2, gn_groups(2, emb), &st);
        ConvArgs r = b.layer("encoder." + std::to_string(2 * nd + 5), t2, 3);
        r.s0.xf = b.gn(st, "encoder." + std::to_string(2 * nd + 3), 2);
        b.conv(r, t3, 0, nullptr);
        b.tap("encoder." + std::to_string(2 * nd + 1), t1); b.tap("encoder." + std::to_string(2 * nd + 2), t2);
        b.tap("encoder." + std::to_string(2 * nd + 5), t3);
    }
    if (b.err) return b.err;
    const float* zp = t3.p;
    const int hw = y.H * y.W;
    b.scope = "z";
    b.push([=](const FwdCtx& cx, hipStream_t s) { return nhwc_to_nchw_launch(zp, cx.out, cx.B, emb, hw, emb, s); }, "nhwc_to_nchw");
    v->enc.maxB = maxB; v->enc.H = H; v->enc.W = W;
    return FC_OK;
}

static int build_decoder(fc_vqvae* v, int maxB, int h, int w) {
    v->dec.release();
    const auto& c = v->c;
    const int nd = c.num_downsamples, emb = c.vq_embedding_dim, hid = c.hidden_channels;
    if (!is_pow2(h) || !is_pow2(w) || h < 4 || w < 4) return fail(FC_E_SHAPE, "vqvae: latent size must be a power of two >= 4");
    if (emb & 3) return fail(FC_E_SHAPE, "vqvae: vq_embedding_dim must be a multiple of 4");
    QBuilder b(v, &v->dec, maxB);
    b.conv_prec = v->prec; b.keep_all = v->taps != 0;
    const std::string L = "decoder.layers.";
    Act z = b.act(emb, h, w);
    float* zp = z.p;
    b.scope = "input";
    b.push([=](const FwdCtx& cx, hipStream_t s) { return nchw_to_nhwc_launch(cx.x, zp, cx.B, emb, h * w, emb, cx.B, s); }, "nchw_to_nhwc");
    int i = 0;
    if (c.decoder_nonlocal) {   // SpatialNonLocalAttention(vq_embedding_dim), codecs.py:252
        Act z2 = b.act(emb, h, w);
        const float *wq = v->R(L + "0.q_proj.weight"), *bq = v->R(L + "0.q_proj.bias"), *wk = v->R(L + "0.k_proj.weight"), *bk = v->R(L + "0.k_proj.bias");
        const float *wv = v->R(L + "0.v_proj.weight"), *bv = v->R(L + "0.v_proj.bias"), *wo = v->R(L + "0.out_proj.weight"), *bo = v->R(L + "0.out_proj.bias");
        float* op = z2.p; const float* ip = z.p;
        const int n = h * w, cr = emb / 2 > 1 ? emb / 2 : 1;
        b.scope = L + "0";
        b.push([=](const FwdCtx& cx, hipStream_t s) { return rope_attn_launch(ip, wq, bq, wk, bk, wv, bv, wo, bo, op, cx.B, n, emb, cr, s); }, "rope_attn");
        b.tap(b.scope, z2);
        z = z2;
        i = 1;
    }
    int cur = hid << (nd - 1);
    Act t1 = b.act(c.internal_dim, h, w), x = b.act(cur, h, w);
    Stat st;
    {
        b.scope = L + std::to_string(i);
        b.conv(b.layer(L + std::to_string(i), z, 1), t1, gn_groups(emb, c.internal_dim), &st);
        ConvArgs q = b.layer(L + std::to_string(i + 3), t1, 1);
        q.s0.xf = b.gn(st, L + std::to_string(i + 1), 2);
        b.conv(q, x, 0, nullptr);
        b.tap(L + std::to_string(i), t1); b.tap(L + std::to_string(i + 3), x);
    }
    if (b.err) return b.err;
    {
        Act y = b.block(L + std::to_string(i + 5), x, cur, 1);
        b.release(x);
        x = y;
    }
    i += 6;
    for (int lvl = nd - 1; lvl >= 0 && !b.err; --lvl) {
        int co = hid << (lvl - 1 > 0 ? lvl - 1 : 0);
        if (lvl == 0) co = hid;
        b.scope = L + std::to_string(i);
        Act u = b.act(4 * cur, x.H, x.W), ps = b.act(cur, 2 * x.H, 2 * x.W);
        ConvArgs a = b.layer(L + std::to_string(i), x, 3);
        a.out_act = 1;                                                                              // conv, SiLU
        b.conv(a, u, 0, nullptr);
        const float* up = u.p; float* pp = ps.p;
        const int Hs = x.H, Ws = x.W, cc = cur;
        b.push([=](const FwdCtx& cx, hipStream_t s) { return pixel_shuffle2_nhwc_launch(up, pp, cx.B, Hs, Ws, cc, s); }, "pixel_shuffle");
        b.tap(L + std::to_string(i), u); b.tap(L + std::to_string(i + 2), ps);   // conv with its SiLU epilogue; nn.PixelShuffle is layer i + 2
        b.release(x); b.release(u);
        Act y1 = b.block(L + std::to_string(i + 4), ps, co, 1);
        b.release(ps);
        Act y2 = b.block(L + std::to_string(i + 6), y1, co, 1);
        b.release(y1);
        x = y2; cur = co;
        i += 7;
    }
    if (b.err) return b.err;
    const int ic = c.in_channels, icp = pad4(ic);
    Act f1 = b.act(64, x.H, x.W), f2 = b.act(icp, x.H, x.W);
    {
        b.scope = "decoder.final";
        ConvArgs a = b.layer(L + std::to_string(i + 1), x, 3);
        a.out_act = 1;
        b.conv(a, f1, 0, nullptr);
        b.conv(b.layer(L + std::to_string(i + 4), f1, 3), f2, 0, nullptr);
        b.tap(L + std::to_string(i + 1), f1); b.tap(L + std::to_string(i + 4), f2);   // f1 with its SiLU epilogue
    }
    if (b.err) return b.err;
    const float* yp = f2.p;
    const int HW = x.H * x.W;
    b.scope = "recon";
    b.push([=](const FwdCtx& cx, hipStream_t s) { return nhwc_to_nchw_launch(yp, cx.out, cx.B, ic, HW, icp, s); }, "nhwc_to_nchw");
    v->dec.maxB = maxB; v->dec.H = h; v->dec.W = w;
    return FC_OK;
}

}  // namespace fc

extern "C" {

int fc_vqvae_create_ex(int in_channels, int hidden_channels, int num_downsamples, int internal_dim, int vq_embedding_dim, int decoder_nonlocal,
                       int natten_layout, int device, fc_vqvae** out) {
    if (!out || in_channels < 1 || hidden_channels < 8 || num_downsamples < 1 || num_downsamples > 6 || internal_dim < 4 || vq_embedding_dim < 1)
        return fail(FC_E_ARG, "fc_vqvae_create: bad config");
    if (natten_layout < 0 || natten_layout > 2) return fail(FC_E_ARG, "fc_vqvae_create: natten_layout must be 0 (no NATTEN blocks), 1 or 2");
    if ((hidden_channels & 3) || (internal_dim & 3) || (vq_embedding_dim & 3)) return fail(FC_E_SHAPE, "vqvae: hidden, internal and embedding widths must be multiples of 4");
    if (natten_layout && ((hidden_channels % 32) || (internal_dim % 32)))
        return fail(FC_E_SHAPE, "vqvae: NATTEN blocks need widths that are multiples of 32 (8 heads, head_dim a multiple of 4)");
    std::unique_ptr<fc_vqvae> v(new fc_vqvae);
    v->c = {in_channels, hidden_channels, num_downsamples, internal_dim, vq_embedding_dim, decoder_nonlocal, natten_layout};
    return codec_create(std::move(v), device, declare_all, out);
}
int fc_vqvae_create(int in_channels, int hidden_channels, int num_downsamples, int internal_dim, int vq_embedding_dim, int decoder_nonlocal,
                    int device, fc_vqvae** out) {
    return fc_vqvae_create_ex(in_channels, hidden_channels, num_downsamples, internal_dim, vq_embedding_dim, decoder_nonlocal, 0, device, out);
}
void fc_vqvae_destroy(fc_vqvae* v) { codec_destroy(v); }
int fc_vqvae_param_count(const fc_vqvae* v) { return v ? (int)v->params.size() : 0; }
int64_t fc_vqvae_param_numel(const fc_vqvae* v) { return v ? v->raw_numel : 0; }
int fc_vqvae_param_info(const fc_vqvae* v, int i, const char** name, int64_t shape[4], int64_t* offset) {
    if (!v) return fail(FC_E_ARG, "fc_vqvae_param_info: null handle");
    return v->info(i, name, shape, offset);
}
int fc_vqvae_load_params(fc_vqvae* v, const float* flat, int64_t numel, int on_device, void* stream) {
    return codec_load(v, "fc_vqvae_load_params", flat, numel, on_device, stream);
}
int fc_vqvae_set_precision(fc_vqvae* v, int mode) { return codec_set_precision(v, "fc_vqvae_set_precision", mode); }
int fc_vqvae_debug_taps(fc_vqvae* v, int on) { return codec_debug_taps(v, "fc_vqvae_debug_taps", on); }
int fc_vqvae_debug_tensor(const fc_vqvae* v, int decode, const char* name, const float** ptr, int* C, int* H, int* W) {
    return codec_debug_tensor(v, "fc_vqvae_debug_tensor", decode, name, ptr, C, H, W);
}
int fc_vqvae_reserve_encode(fc_vqvae* v, int max_batch, int height, int width) {
    return codec_reserve(v, "fc_vqvae_reserve_encode", 0, build_encoder, max_batch, height, width);
}
int fc_vqvae_reserve_decode(fc_vqvae* v, int max_batch, int lat_height, int lat_width) {
    return codec_reserve(v, "fc_vqvae_reserve_decode", 1, build_decoder, max_batch, lat_height, lat_width);
}
int fc_vqvae_encode(fc_vqvae* v, const float* x_dev, float* z_out_dev, int batch, int height, int width, void* stream) {
    return codec_run(v, "fc_vqvae_encode", 0, x_dev, z_out_dev, batch, height, width, stream);
}
int fc_vqvae_decode(fc_vqvae* v, const float* z_dev, float* x_out_dev, int batch, int lat_height, int lat_width, void* stream) {
    return codec_run(v, "fc_vqvae_decode", 1, z_dev, x_out_dev, batch, lat_height, lat_width, stream);
}
double fc_vqvae_flops_per_sample(const fc_vqvae* v, int decode) { return v ? v->plan(decode).flops : 0.0; }
int fc_vqvae_plan_launches(const fc_vqvae* v, int decode) { return v ? (int)v->plan(decode).ops.size() : 0; }
int fc_vqvae_op_info(const fc_vqvae* v, int decode, int i, const char** kernel, const char** module, double* flops_per_sample,
                     double* bytes_per_sample, double* bytes_per_launch) {
    return codec_op_info(v, "fc_vqvae_op_info", decode, i, kernel, module, flops_per_sample, bytes_per_sample, bytes_per_launch);
}
int fc_vqvae_profile_ops(fc_vqvae* v, int decode, const float* in_dev, float* out_dev, int batch, int repeats, float* ms_out, int n_out, void* stream) {
    return codec_profile(v, "fc_vqvae_profile_ops", decode, in_dev, out_dev, batch, repeats, ms_out, n_out, stream);
}

}  // extern "C"
