// Native runtime of the velocity U-Net: parameter table with the reference's state_dict names, weight
// packing, a static launch plan over a fixed activation arena, and the hipGraph-captured ODE step.
//
// Topology follows Unet._forward (unet.py:289-372); every kernel launch below cites the reference lines it
// covers.  The plan is built once per (max_batch, H, W) -- buffers never move, so one integration step can be
// captured in a hipGraph and replayed (the reference's per-call host syncs are gone).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "plan.h"
#include "unet_priv.h"
#include "unet_sample.h"
#include "unet_walk.h"

namespace fc {

static thread_local std::string g_err;
void set_error(const std::string& m) { g_err = m; }
int fail(int code, const std::string& m) { g_err = m; return code; }
const char* last_error() { return g_err.c_str(); }

}  // namespace fc

using namespace fc;

namespace fc {

// ------------------------------------------------------------------------------------------- parameters
static void declare(fc_unet* u, const std::string& name, std::initializer_list<int64_t> shape) { u->declare(name, shape); }
static int64_t pk_alloc(fc_unet* u, const std::string& name, int64_t numel) { return u->pk_alloc(name, numel); }
static void decl_conv(fc_unet* u, const std::string& n, int O, int I, int K, bool bias = true) { u->decl_conv(n, O, I, K, bias); }
static void decl_linear_t(fc_unet* u, const std::string& n, int O, int I) { u->decl_linear_t(n, O, I); }
static void decl_norm(fc_unet* u, const std::string& n, int C) { u->decl_norm(n, C); }
static void decl_resblock(fc_unet* u, const std::string& p, int cin, int cout) {
    declare(u, p + ".mlp.1.weight", {2 * cout, u->td});
    declare(u, p + ".mlp.1.bias", {2 * cout});
    u->ss_off[p] = u->S;
    u->S += 2 * cout;
    decl_conv(u, p + ".block1.proj", cout, cin, 3);
    decl_norm(u, p + ".block1.norm", cout);
    decl_conv(u, p + ".block2.proj", cout, cout, 3);
    decl_norm(u, p + ".block2.norm", cout);
    if (cin != cout) decl_conv(u, p + ".res_conv", cout, cin, 1);
}
static void decl_linattn(fc_unet* u, const std::string& p, int C) {
    const int hid = u->heads * 32;
    decl_conv(u, p + ".fn.fn.to_qkv", 3 * hid, C, 1, false);   // PreNorm registers fn before norm (unet.py:156-157)
    decl_conv(u, p + ".fn.fn.to_out.0", C, hid, 1);
    decl_norm(u, p + ".fn.fn.to_out.1", C);
    decl_norm(u, p + ".fn.norm", C);
}

// PyTorch's registration order (ups before mid_*), not walk_unet's execution order: every parameter's offset in the flat table pins it
static int declare_all(fc_unet* u) {
    const fc_unet_config& c = u->cfg;
    const int dim = c.dim, ch = c.channels, L = c.n_levels;
    u->td = dim * 8;  // unet.py:197
    u->chans.assign(1, dim);
    for (int i = 0; i < L; ++i) u->chans.push_back(dim * c.dim_mults[i]);
    const std::vector<int>& cs = u->chans;
    decl_conv(u, "init_conv", dim, ch, 1);
    decl_linear_t(u, "time_mlp.1", u->td, dim);
    decl_linear_t(u, "time_mlp.3", u->td, u->td);
    if (c.n_classes > 0) {
        declare(u, "class_cond_mlp.0.weight", {c.n_classes, u->td});
        decl_linear_t(u, "class_cond_mlp.1", u->td, u->td);
        decl_linear_t(u, "class_cond_mlp.3", u->td, u->td);
    }
    if (c.mask_cond) {  // unet.py:214-235
        decl_conv(u, "mask_fusion_conv.0", 2 * dim, dim + ch, 5);
        decl_conv(u, "mask_fusion_conv.2", 2 * dim, 2 * dim, 3);
        decl_conv(u, "mask_fusion_conv.4", dim, 2 * dim, 3);
        for (int i = 0; i < 2 && i < L; ++i) decl_conv(u, "down_mask_fusions." + std::to_string(i) + ".0", cs[i], cs[i] + ch, 3);
        for (int i = 0; i < 2 && i < L; ++i) decl_conv(u, "up_mask_fusions." + std::to_string(i) + ".0", cs[L - i], cs[L - i] + ch, 3);
    }
    for (int i = 0; i < L; ++i) {  // unet.py:242-258
        const std::string p = "downs." + std::to_string(i);
        decl_resblock(u, p + ".0", cs[i], cs[i]);
        decl_resblock(u, p + ".1", cs[i], cs[i]);
        decl_linattn(u, p + ".2", cs[i]);
        if (i == L - 1) decl_conv(u, p + ".3", cs[i + 1], cs[i], 3);
        else u->decl_conv_s2d(p + ".3.1", cs[i + 1], cs[i]);
    }
    for (int i = 0; i < L; ++i) {  // unet.py:265-281, (dim_in, dim_out) = reversed(in_out)[i]
        const std::string p = "ups." + std::to_string(i);
        const int din = cs[L - 1 - i], dout = cs[L - i];
        decl_resblock(u, p + ".0", dout + din, dout);
        decl_resblock(u, p + ".1", dout + din, dout);
        decl_linattn(u, p + ".2", dout);
        if (i == L - 1) decl_conv(u, p + ".3", din, dout, 3);
        else u->decl_conv_up2(p + ".3.1", din, dout);      // Upsample: also the four parity kernels of the folded form (plan.h conv_up2)
    }
    const int mid = cs[L];
    decl_resblock(u, "mid_block1", mid, mid);
    decl_conv(u, "mid_attn.fn.fn.to_qkv", 3 * u->heads * 32, mid, 1, false);
    decl_conv(u, "mid_attn.fn.fn.to_out", mid, u->heads * 32, 1);
    decl_norm(u, "mid_attn.fn.norm", mid);
    decl_resblock(u, "mid_block2", mid, mid);
    decl_resblock(u, "final_res_block", 2 * dim, dim);
    decl_conv(u, "final_conv", ch, dim, 1);
    // concatenated scale/shift projection of every ResnetBlock: wt [td][S], bias [S]
    pk_alloc(u, "__ss_wt", (int64_t)u->td * u->S);
    pk_alloc(u, "__ss_bias", u->S);
    for (auto& kv : u->ss_off) {
        const int n = (int)u->params[u->pidx[kv.first + ".mlp.1.bias"]].numel;     // 2 * cout
        u->pack_transpose_into("__ss_wt", kv.first + ".mlp.1.weight", n, u->td, u->S, kv.second);
        u->pack_copy_into("__ss_bias", kv.first + ".mlp.1.bias", n, kv.second);
    }
    return FC_OK;
}

// Fused Block tails across workgroups (ConvFin): on by default since the meeting became one tagged-granule round trip (+2.5 % on the
// sampler, profiles/r02_*).  fc_debug_set_fused_tail: -1 default (on), 0 no meeting launches (the tile-local form stays), 1 on.
static int g_fused_tail = -1;
static bool fused_tail_enabled() { return g_fused_tail != 0; }

// ------------------------------------------------------------------------------------------- plan builder
// Arithmetic of one attention module per sample: to_qkv, the two products of the core (linear: 32x32 contexts per head; full: n x n scores), to_out
static double attn_flops(int n, int C, int heads, bool full) {
    const int hid = heads * 32;
    return 2.0 * n * (double)C * 3 * hid + (full ? 2.0 * 2.0 * n * n * 32 * heads : 2.0 * 2 * n * 32 * 32 * heads) + 2.0 * n * (double)hid * C;
}

// The ordinary plan: walk_unet's emitter of one launch (or a few) per module over arena tensors.  Every activation keeps a buffer of its
// own (retire does nothing): debug taps and the backward read them after the forward.
struct Builder : PlanBuilder {
    using T = Act;
    fc_unet* u = nullptr;
    const int H, W;           // the latent's extent
    Act mask_nhwc;            // stem: the call's mask as the injections read it
    Stat gn1;                 // GroupNorm(1) statistics a resblock(..., feeds_attention) leaves of its output: the following attention's PreNorm
    Builder(fc_unet* u_, Plan* pl_, int B_, int H_, int W_) : u(u_), H(H_), W(W_) { pl = pl_; B = B_; fin_err_word = u_->dev_err; store = u_; }
    // launches that wait for other workgroups: only on a device this handle has to itself
    bool meeting_ok() const { return fused_tail_enabled() && !u->shared; }
    void retire(const Act&) {}

    // ResnetBlock (unet.py:76-96): conv1 [+res_conv] | conv2 with GN+FiLM+SiLU folded into its loader | finalize.
    Act resblock(const std::string& p, const Act& x, const Act* skip, int cout, bool feeds_attention) {
        scope = p;
        const int G = u->cfg.groups, cin = x.C + (skip ? skip->C : 0);
        Act h1 = act(cout, x.H, x.W), h2 = act(cout, x.H, x.W), out = act(cout, x.H, x.W), rb;
        Stat st1, st2;
        ConvArgs a = layer(p + ".block1.proj", x, 3);
        if (skip) a.s1 = src(*skip);
        a.w4 = u->P8(p + ".block1.proj.weight");
        if (cin != cout) {
            rb = act(cout, x.H, x.W);
            a.res_w = u->P(p + ".res_conv.weight"); a.res_b = u->R(p + ".res_conv.bias"); a.res_out = rb.p;
            a.res_w4 = u->P8(p + ".res_conv.weight");
            if (!a.res_w4) a.w4 = nullptr;      // both operands or neither
        }
        conv(a, h1, G, &st1);
        ConvArgs b = layer(p + ".block2.proj", h1, 3);
        b.s0.xf = xf_of(st1, 2, u->R(p + ".block1.norm.weight"), u->R(p + ".block1.norm.bias"), pl->ss + u->ss_off.at(p), u->S);
        b.w4 = u->P8(p + ".block2.proj.weight");
        // Inference plans close the Block inside conv2 (ConvFin) when the launch keeps its whole grid resident: across workgroups where
        // meeting launches are allowed (meeting_ok), and always where a tile holds whole GroupNorm groups (dim 32: the 128-channel blocks
        // at 4x4 and 8x8, 32 channels per group) and there is nothing to meet for.  Training plans keep the raw h2 and its statistics for
        // the backward: conv + finalize (a fused training tail measured no faster, r02: stl_sd step 3.515 against 3.446 ms).
        const float* resp = (cin != cout) ? rb.p : x.p;
        const bool fused = !u->keep_all &&
                           conv_fin(b, out, G, u->R(p + ".block2.norm.weight"), u->R(p + ".block2.norm.bias"), resp, feeds_attention, &gn1, !meeting_ok());
        if (!fused) {
            conv(b, h2, G, &st2);
            FinalizeArgs f = fin_of(h2, xf_of(st2, 2, u->R(p + ".block2.norm.weight"), u->R(p + ".block2.norm.bias")), out);
            f.res = resp;
            if (feeds_attention) {
                const int bps = finalize_blocks_per_sample(f.HW, f.C);
                gn1 = stat(1, bps, (float)(f.HW * f.C / bps));
                f.stats_out = gn1.p;
            }
            finalize(f);
        }
        pl->named[p] = out; pl->named[p + ".h1"] = h1; pl->named[p + ".h2"] = h2;
        ResRec rec;
        rec.p = p; rec.x = x; if (skip) rec.skip = *skip; rec.h1 = h1; rec.h2 = h2; rec.rb = rb; rec.out = out; rec.st1 = st1; rec.st2 = st2; rec.cout = cout;
        pl->tape.push_back({TAPE_RES, (int)pl->res.size()});
        pl->res.push_back(rec);
        return out;
    }

    // Residual(PreNorm(LinearAttention)) (unet.py:125-161,250): qkv conv with GroupNorm(1) in its loader | context |
    // apply | to_out conv | GroupNorm(1) + residual.
    Act attention(const std::string& p, const Act& x, bool full) {
        scope = p;
        if (full) return midattn(p, x);
        const int hid = u->heads * 32, n = x.H * x.W, heads = u->heads;
        // measured (tools/op_table.py, B=64): fused 110 vs 201 us at n=1024, 43 vs 65 us at n=256; at n <= 64 the per-workgroup weight
        // loads dominate and the unfused chain wins (37 vs 67 us at n=16, C=256)
        if (!u->keep_all && n >= 256 && linattn_fused_supported(n, x.C, heads)) return linattn_fused(p, x);
        // n <= 64: a workgroup per (sample, head), then one per sample (linattn_sample.hip): 2 launches instead of 5
        if (!u->keep_all && linattn_sample_supported(n, x.C, heads)) return attn_sample(p, x, false);
        Act qkv = act(3 * hid, x.H, x.W), lao = act(hid, x.H, x.W), yb = act(x.C, x.H, x.W), out = act(x.C, x.H, x.W);
        float* ctx = dmalloc((size_t)B * heads * 32 * 32);
        ConvArgs a = layer(p + ".fn.fn.to_qkv", x, 1);
        a.s0.xf = xf_of(gn1, 1, u->R(p + ".fn.norm.weight"), u->R(p + ".fn.norm.bias"));
        conv(a, qkv, 0, nullptr);
        const float* qp = qkv.p; float* lp = lao.p;
        if (!err) {
            push([=](const FwdCtx& c, hipStream_t s) { return linattn_ctx_launch(qp, ctx, c.B, n, heads, s); }, "linattn_ctx", 2.0 * n * 32 * 32 * heads);
            push([=](const FwdCtx& c, hipStream_t s) { return linattn_apply_launch(qp, ctx, lp, c.B, n, heads, s); }, "linattn_apply", 2.0 * n * 32 * 32 * heads);
        }
        Stat sty;
        conv(layer(p + ".fn.fn.to_out.0", lao, 1), yb, 1, &sty);
        FinalizeArgs f = fin_of(yb, xf_of(sty, 1, u->R(p + ".fn.fn.to_out.1.weight"), u->R(p + ".fn.fn.to_out.1.bias")), out);
        f.res = x.p;
        finalize(f);
        pl->named[p] = out; pl->named[p + ".qkv"] = qkv; pl->named[p + ".lao"] = lao; pl->named[p + ".y"] = yb;
        LinRec rec;
        rec.p = p; rec.x = x; rec.qkv = qkv; rec.lao = lao; rec.yb = yb; rec.out = out; rec.ctx = ctx; rec.gn1 = gn1; rec.sty = sty;
        pl->tape.push_back({TAPE_LIN, (int)pl->lin.size()});
        pl->lin.push_back(rec);
        return out;
    }

    // what the three one- and two-launch attention forms fill alike; `full`: mid_attn's to_out is a bare convolution (unet.py:112), no Sequential
    LaArgs la_args(const std::string& p, const Act& x, bool full) const {
        const std::string to_out = p + (full ? ".fn.fn.to_out" : ".fn.fn.to_out.0");
        LaArgs a;
        a.x = x.p; a.xf = xf_of(gn1, 1, u->R(p + ".fn.norm.weight"), u->R(p + ".fn.norm.bias"));
        a.wqkv = u->P(p + ".fn.fn.to_qkv.weight"); a.wout = u->P(to_out + ".weight"); a.bout = u->R(to_out + ".bias");
        a.n = x.H * x.W; a.C = x.C; a.heads = u->heads;
        return a;
    }

    // the same module on the fused kernels (linattn_fused.hip): x -> context -> y in two launches, q/k/v never stored
    Act linattn_fused(const std::string& p, const Act& x) {
        const int n = x.H * x.W, heads = u->heads;
        Act yb = act(x.C, x.H, x.W), out = act(x.C, x.H, x.W);
        Stat sty = stat(1, linattn_fused_tiles(n), linattn_fused_nt(n, x.C));
        LaArgs a = la_args(p, x, false);
        a.ctx = dmalloc((size_t)B * heads * 32 * 32); a.y = yb.p; a.stats_out = sty.p;
        const double fl = attn_flops(n, x.C, heads, false);
        // The module closed by its own apply launch (to_out.1's GroupNorm(1) + the residual on the tile still in registers: no y round trip,
        // no finalize launch) where the workgroups of a sample may wait for each other: the exclusive plan, the whole grid resident.
        if (!err && meeting_ok() && linattn_fused_meeting_ok(B, n, x.C)) {
            const int T = linattn_fused_tiles(n);
            a.g2 = u->R(p + ".fn.fn.to_out.1.weight"); a.b2 = u->R(p + ".fn.fn.to_out.1.bias"); a.out = out.p;
            a.gran = reinterpret_cast<unsigned long long*>(dmalloc((size_t)B * T * 2 * 2));
            a.sync = reinterpret_cast<unsigned*>(dmalloc((size_t)B));
            if (err) return out;
            if (hipMemset(a.gran, 0, (size_t)B * T * 2 * sizeof(unsigned long long)) != hipSuccess || hipMemset(a.sync, 0, (size_t)B * sizeof(unsigned)) != hipSuccess) {
                err = fail(FC_E_HIP, "hipMemset failed");
                return out;
            }
            a.err = fin_err_word;
            ++pl->n_meet; pl->fin_sync.push_back(a.sync); pl->fin_kind.push_back(1);
            push([a](const FwdCtx& c, hipStream_t s) { LaArgs b = a; b.B = c.B; return linattn_fused_launch(b, s); }, "linattn_fused+fin", fl);
            pl->named[p] = out;
            return out;
        }
        if (!err) push([a](const FwdCtx& c, hipStream_t s) { LaArgs b = a; b.B = c.B; return linattn_fused_launch(b, s); }, "linattn_fused", fl);
        FinalizeArgs f = fin_of(yb, xf_of(sty, 1, u->R(p + ".fn.fn.to_out.1.weight"), u->R(p + ".fn.fn.to_out.1.bias")), out);
        f.res = x.p;
        finalize(f);
        pl->named[p] = out; pl->named[p + ".y"] = yb;
        return out;
    }

    // the whole module, linear or full, in two launches (linattn_sample.hip)
    Act attn_sample(const std::string& p, const Act& x, bool full) {
        const int n = x.H * x.W, heads = u->heads;
        Act out = act(x.C, x.H, x.W);
        LaArgs a = la_args(p, x, full);
        a.wqkv4 = u->P8(p + ".fn.fn.to_qkv.weight");
        if (!full) { a.g2 = u->R(p + ".fn.fn.to_out.1.weight"); a.b2 = u->R(p + ".fn.fn.to_out.1.bias"); }
        a.out = out.p;
        a.part = dmalloc((size_t)B * heads * n * x.C);
        if (!err) push([a, full](const FwdCtx& c, hipStream_t s) { LaArgs b = a; b.B = c.B; return full ? attn_sample_launch(b, s) : linattn_sample_launch(b, s); },
                       full ? "attn_sample" : "linattn_sample", attn_flops(n, x.C, heads, full));
        pl->named[p] = out;
        return out;
    }

    // Residual(PreNorm(Attention)) (unet.py:99-122,262)
    Act midattn(const std::string& p, const Act& x) {
        const int hid = u->heads * 32, n = x.H * x.W, heads = u->heads;
        if (!u->keep_all && attn_sample_supported(n, x.C, heads)) return attn_sample(p, x, true);    // two launches instead of three
        Act qkv = act(3 * hid, x.H, x.W), ao = act(hid, x.H, x.W), out = act(x.C, x.H, x.W);
        ConvArgs a = layer(p + ".fn.fn.to_qkv", x, 1);
        a.s0.xf = xf_of(gn1, 1, u->R(p + ".fn.norm.weight"), u->R(p + ".fn.norm.bias"));
        conv(a, qkv, 0, nullptr);
        const float* qp = qkv.p; float* ap = ao.p;
        if (!err) {
            push([=](const FwdCtx& c, hipStream_t s) { return attn_small_launch(qp, ap, c.B, n, heads, s); }, "attn_small", 2.0 * 2.0 * n * n * 32 * heads);
        }
        ConvArgs o = layer(p + ".fn.fn.to_out", ao, 1);
        o.add = x.p;
        conv(o, out, 0, nullptr);
        pl->named[p] = out;
        MidRec rec;
        rec.x = x; rec.qkv = qkv; rec.ao = ao; rec.out = out; rec.gn1 = gn1;
        pl->tape.push_back({TAPE_MID, (int)pl->mid.size()});
        pl->mid.push_back(rec);
        return out;
    }

    // x + SiLU(conv3x3(cat[x, bilinear(mask)]))  (unet.py:336-340,360-364); a plain copy when no mask is given
    Act inject(const std::string& name, const Act& x) {
        scope = name;
        Act mr = act(mask_nhwc.C, x.H, x.W), out = act(x.C, x.H, x.W);
        if (err) return out;
        const float* mp = mask_nhwc.p; float* rp = mr.p;
        const int C = mask_nhwc.C, Hs = mask_nhwc.H, Ws = mask_nhwc.W, Hd = x.H, Wd = x.W;
        const bool keep = u->keep_all;             // training: the pre-activation z stays (SiLU' needs it), SiLU + residual as a pass of its own
        Act z = keep ? act(x.C, x.H, x.W) : Act();
        ConvArgs a = layer(name, x, 3);
        a.s1 = src(mr);
        if (!keep) { a.out_act = 1; a.add = x.p; }
        bind_out(a, keep ? z : out);
        ConvGeom g;
        if ((err = conv_plan(a, TILE_AUTO, &g)) != FC_OK) return out;
        const int tile = g.tile;
        const size_t per = (size_t)x.H * x.W * x.C;
        const float* xp = x.p; float* op = out.p; const float* zp = z.p;
        push([=](const FwdCtx& c, hipStream_t s) -> int {
            if (!c.mask) { FC_HIP(hipMemcpyAsync(op, xp, per * sizeof(float) * c.B, hipMemcpyDeviceToDevice, s)); return FC_OK; }
            FC_TRY(bilinear_nhwc_launch(mp, rp, c.B, C, Hs, Ws, Hd, Wd, s));
            ConvArgs b = a; b.B = c.B;
            FC_TRY(conv_launch(b, tile, s));
            return keep ? silu_fwd_launch(zp, xp, op, per * c.B, s) : FC_OK;
        }, std::string("bilinear+") + kTileNames[tile], 2.0 * x.H * x.W * 9 * (double)a.Cin * a.Cout);
        InjRec rec;
        rec.name = name; rec.x = x; rec.mr = mr; rec.z = z; rec.out = out;
        pl->tape.push_back({TAPE_INJ, (int)pl->inj.size()});
        pl->inj.push_back(rec);
        return out;
    }

    // init_conv (unet.py:295) and mask fusion (unet.py:298-305)
    Act stem() {
        const fc_unet_config& c = u->cfg;
        const int dim = c.dim, ch = c.channels, HW = H * W;
        Act x0 = act(dim, H, W);
        pl->named["init"] = x0;
        pl->x0 = x0;
        const float *w = u->P("init_conv.weight"), *bias = u->R("init_conv.bias");
        float* x0p = x0.p;
        scope = "init_conv";
        if (!c.mask_cond) {
            // (cx.step: the evaluation before this one has written x0 and fetched the conditioning slice -- conv_dev.h FL_STEP)
            push([=](const FwdCtx& cx, hipStream_t s) { return cx.step ? (int)FC_OK : init_conv_launch(cx.fetch, cx.x, cx.x_mod, w, bias, x0p, cx.B, ch, HW, dim, s); }, "init_conv", 2.0 * HW * ch * dim);
            return x0;
        }
        Act xi = act(dim, H, W), f1 = act(2 * dim, H, W), f2 = act(2 * dim, H, W);
        const bool keep = u->keep_all;         // training keeps the pre-activations z1, z2 of the two SiLU layers
        Act z1 = keep ? act(2 * dim, H, W) : Act(), z2 = keep ? act(2 * dim, H, W) : Act();
        mask_nhwc = act(ch, H, W);
        float *xip = xi.p, *mp = mask_nhwc.p;
        push([=](const FwdCtx& cx, hipStream_t s) -> int {
            if (cx.mask) FC_TRY(nchw_to_nhwc_launch(cx.mask, mp, cx.B, ch, HW, ch, cx.x_mod, s));
            return init_conv_launch(cx.fetch, cx.x, cx.x_mod, w, bias, cx.mask_fuse ? xip : x0p, cx.B, ch, HW, dim, s);
        }, "init_conv", 2.0 * HW * ch * dim);
        ConvArgs a[3];
        const char* names[3] = {"mask_fusion_conv.0", "mask_fusion_conv.2", "mask_fusion_conv.4"};
        const Act* srcs[3] = {&xi, &f1, &f2};
        const Act* dsts[3] = {keep ? &z1 : &f1, keep ? &z2 : &f2, &x0};
        int tiles[3];
        for (int i = 0; i < 3 && !err; ++i) {
            a[i] = layer(names[i], *srcs[i], i == 0 ? 5 : 3);
            if (i == 0) a[i].s1 = src(mask_nhwc);
            a[i].out_act = (i < 2 && !keep);
            bind_out(a[i], *dsts[i]);
            ConvGeom g;
            err = conv_plan(a[i], TILE_AUTO, &g);
            tiles[i] = g.tile;
        }
        if (err) return x0;
        const ConvArgs a0 = a[0], a1 = a[1], a2 = a[2];
        const int t0 = tiles[0], t1 = tiles[1], t2 = tiles[2];
        const float *z1p = z1.p, *z2p = z2.p;
        float *f1p = f1.p, *f2p = f2.p;
        const size_t nf = (size_t)HW * 2 * dim;
        scope = "mask_fusion_conv";
        push([=](const FwdCtx& cx, hipStream_t s) -> int {
            if (!cx.mask_fuse) return FC_OK;
            ConvArgs q = a0; q.B = cx.B; FC_TRY(conv_launch(q, t0, s));
            if (keep) FC_TRY(silu_fwd_launch(z1p, nullptr, f1p, nf * cx.B, s));
            q = a1; q.B = cx.B; FC_TRY(conv_launch(q, t1, s));
            if (keep) FC_TRY(silu_fwd_launch(z2p, nullptr, f2p, nf * cx.B, s));
            q = a2; q.B = cx.B; return conv_launch(q, t2, s);
        }, "mask_fusion(3 x conv_igemm)", 2.0 * HW * (25.0 * (dim + ch) * 2 * dim + 9.0 * 2 * dim * 2 * dim + 9.0 * 2 * dim * dim));
        pl->fuse.present = true;
        pl->fuse.xi = xi; pl->fuse.mask = mask_nhwc; pl->fuse.z1 = z1; pl->fuse.f1 = f1; pl->fuse.z2 = z2; pl->fuse.f2 = f2; pl->fuse.x0 = x0;
        return x0;
    }

    // downs.i.3 / ups.i.3: Downsample, a 2x2 / stride-2 convolution (unet.py:253); Upsample, nearest x2 + 3x3 (unet.py:42-46); on the last
    // level a 3x3 convolution that keeps the resolution
    Act resample(const std::string& p, const Act& x, int cout, bool last, bool up) {
        scope = p;
        const std::string name = last ? p : p + ".1";
        const bool down = !last && !up;
        ConvArgs a = layer(name, x, down ? 2 : 3);
        if (down) { a.pad = 0; a.stride = 2; }
        a.ups = !last && up;
        a.w4 = u->P8(name + ".weight");    // (no k-step-quad copy of a Downsample's weight)
        Act o = down ? act(cout, x.H / 2, x.W / 2) : act(cout, x.H << a.ups, x.W << a.ups);
        // (round 3) the upsampling folded into the WEIGHTS -- four 2x2 parity convolutions on x in one launch, 4/9 of the multiply-adds
        // (plan.h conv_up2; FLOCODER_AMD_UPS_FOLD=0: off).  Training plans too: it is the same function of (x, w) up to fp32 rounding, and
        // the backward differentiates it in its 3x3 form from the same saved x (flowers-sized step 6.49 -> 6.45 ms).  Where the shape is
        // not covered, nn.Upsample folded into the convolution's loader.
        if (!a.ups || !conv_up2(x, u->PUP(name + ".weight"), a.bias, o, 0, nullptr)) conv(a, o, 0, nullptr);
        pl->tape.push_back({TAPE_CONV, (int)pl->convs.size()});
        pl->convs.push_back({name, x, o, a.KS, a.pad, a.stride, a.ups});
        pl->named[p] = o;
        return o;
    }
    Act downsample(const std::string& p, const Act& x, int cout, bool last) { return resample(p, x, cout, last, false); }
    Act upsample(const std::string& p, const Act& x, int cout, bool last) { return resample(p, x, cout, last, true); }

    // final_res_block on cat[x, x0] and final_conv (unet.py:369-372)
    Act head(const Act& x, const Act& x0) {
        const fc_unet_config& c = u->cfg;
        const int dim = c.dim, ch = c.channels, HW = H * W;
        // final_res_block's closing launch may close the Euler sampler's step as well: final_conv, the update and the next evaluation's
        // init_conv are pointwise per pixel (init_conv is a 1x1 convolution here), and the launch's tile holds every channel of its pixels
        if (!c.mask_cond && dim == kStepDim && ch == kStepCh) step_out = x0;
        pl->head = resblock("final_res_block", x, &x0, dim, false);
        step_out = Act();
        const float *xp = pl->head.p, *w = u->P("final_conv.weight"), *bias = u->R("final_conv.bias");
        scope = "final_conv";
        if (!err) push([=](const FwdCtx& cx, hipStream_t s) { return cx.step ? (int)FC_OK : final_conv_launch(xp, w, bias, cx.out, cx.B, dim, HW, ch, cx.euler, s); }, "final_conv", 2.0 * HW * dim * ch);
        return Act();             // final_conv writes the caller's tensor (FwdCtx::out), not the arena
    }
};

static void free_plan(fc_unet* u) {
    u->ig.release_plan();                   // the captured graphs first: they bake the addresses of the buffers they were captured with
    u->plan.release();
    u->bwd.release();                       // the backward plan points into the forward arena
    u->dgrad_packs.clear();
    u->dgrad_table.release();
    u->maxB = 0;
    // a rebuilt plan starts clean (callers of free_plan have synchronised the device)
    if (u->dev_err) (void)hipMemset(u->dev_err, 0, sizeof(int));
    if (u->host_err) *u->host_err = 0;
    u->tail_failed = false;
}

// ---- one workgroup per sample (unet_sample.hip): the forward as a program over LDS-resident activations -------------------------------
// Used for inference plans of models whose whole per-sample state fits a CU's LDS (the dim-8 inpainting flow at 4x8x8: BASELINE config 5).
// SampleProgram is walk_unet's emitter of that program: tensors are offsets into the workgroup's LDS, a step is one SStep.
struct SampleProgram {
    struct T { int off = -1, C = 0, H = 0, W = 0; };
    const fc_unet* u;
    const int H, W, dim, ch, G, heads;
    std::vector<SStep> prog;
    int top = 0, peak = 0;
    double flops = 0.0;
    T xin, mask;              // stem: where the launch puts the call's x and mask
    SampleProgram(const fc_unet* u_, int H_, int W_) : u(u_), H(H_), W(W_), dim(u_->cfg.dim), ch(u_->cfg.channels), G(u_->cfg.groups), heads(u_->heads) {}

    int alloc(int floats) { const int o = top; top += (floats + 3) & ~3; if (top > peak) peak = top; return o; }
    // block outputs whose last reader has been emitted serve later tensors of the same size (every tensor a step reads or writes is alive
    // for the whole step, so a buffer may be handed out again only AFTER the step that last read it has been pushed: walk_unet's order)
    std::multimap<int, int> pool;
    T tensor(int C, int h, int w) {
        T t; t.C = C; t.H = h; t.W = w;
        auto it = pool.find(C * h * w);
        if (it != pool.end()) { t.off = it->second; pool.erase(it); }
        else t.off = alloc(C * h * w);
        return t;
    }
    void retire(const T& t) { if (t.off >= 0) pool.emplace(t.C * t.H * t.W, t.off); }
    // a temporary of the running module: stack-allocated above the module's `mark`, never pooled
    T temp(int C, int h, int w) { T t; t.C = C; t.H = h; t.W = w; t.off = alloc(C * h * w); return t; }
    struct NormSpec { std::string name; int groups = 0, ss_off = -1; };       // a GroupNorm folded into the convolution's epilogue (groups > 0)
    // emits the step; returns its FLOPs per sample
    double conv(const T& x, const T* x1, const T& out, const std::string& name, int KS, int pad, int stride, int ups, int act, int res, int guard, bool bias = true,
                const NormSpec* nm = nullptr) {
        SStep s;
        if (nm && nm->groups > 0) {
            s.fnorm = 1; s.G = nm->groups; s.ss_off = nm->ss_off; s.lcpg = ilog2(out.C / nm->groups);
            s.gamma = u->R(nm->name + ".weight"); s.beta = u->R(nm->name + ".bias");
        }
        s.op = S_CONV; s.guard = guard; s.in0 = x.off; s.C0 = x.C; s.in1 = x1 ? x1->off : -1; s.C1 = x1 ? x1->C : 0;
        s.out = out.off; s.Cout = out.C; s.Hi = x.H; s.Wi = x.W; s.Ho = out.H; s.Wo = out.W; s.KS = KS; s.pad = pad; s.stride = stride; s.ups = ups;
        s.act = act; s.res = res; s.w = u->P(name + ".weight"); s.bias = bias ? u->R(name + ".bias") : nullptr;
        s.lco = ilog2(out.C);
        {   // the weight rows some output pixel can reach, merged where contiguous, cut into chunks of <= 4096 floats
            const int Cin = s.C0 + s.C1, Hin = x.H << ups, Win = x.W << ups, RW0 = 4096 / out.C;
            int kx_lo = KS, kx_hi = -1;
            for (int kx = 0; kx < KS; ++kx) if ((out.W - 1) * stride - pad + kx >= 0 && -pad + kx < Win) { if (kx < kx_lo) kx_lo = kx; kx_hi = kx; }
            std::vector<std::pair<int, int>> ranges;
            for (int ky = 0; ky < KS && kx_hi >= kx_lo; ++ky) {
                if (!((out.H - 1) * stride - pad + ky >= 0 && -pad + ky < Hin)) continue;
                const int r0 = (ky * KS + kx_lo) * Cin, r1 = (ky * KS + kx_hi + 1) * Cin;
                if (!ranges.empty() && ranges.back().second == r0) ranges.back().second = r1;
                else ranges.push_back({r0, r1});
            }
            // (whole taps per chunk where a tap's rows fit one; whole channel quads otherwise)
            const int RW = RW0 >= Cin ? (RW0 / Cin) * Cin : (RW0 & ~3);
            int nck = 0;
            for (auto& rg : ranges)
                for (int r = rg.first; r < rg.second; r += RW) {
                    if (nck < 8) { s.crow[nck] = r; s.cn[nck] = rg.second - r < RW ? rg.second - r : RW; }
                    ++nck;
                }
            s.nchunk = nck;                              // > 8: the model does not qualify (checked below)
            // lanes per output quad: as many as fill the workgroup, at most the channel quads of a tap
            const int quads = out.H * out.W * out.C / 4, CQ = Cin / 4;
            while (s.lks < 6 && (quads << (s.lks + 1)) <= SAMPLE_THREADS && (2 << s.lks) <= CQ) ++s.lks;
            // the unrolled multiply-add: ONE chunk of one tap or of all nine taps of a 3x3 kernel, the lanes of a quad dividing a tap's channel
            // quads evenly, at most four each
            const int ntaps = nck == 1 ? s.cn[0] / Cin : 0;
            if (nck == 1 && s.cn[0] == ntaps * Cin && (ntaps == 1 || (ntaps == 9 && KS == 3 && s.crow[0] == 0))) {
                int lf = 0;
                while (lf < 6 && (quads << (lf + 1)) <= SAMPLE_THREADS && CQ % (2 << lf) == 0) ++lf;
                if (CQ >> lf <= 4) { s.lks = lf; s.nqi = CQ >> lf; s.fast = ntaps; }
            }
        }
        prog.push_back(s);
        return 2.0 * out.H * out.W * KS * KS * (double)(s.C0 + s.C1) * out.C;
    }
    void copy(const T& x, const T& out, int guard) {
        SStep s;
        s.op = S_COPY; s.guard = guard; s.in0 = x.off; s.out = out.off; s.Cout = x.C * x.H * x.W;
        prog.push_back(s);
    }
    T resblock(const std::string& p, const T& x, const T* skip, int cout, bool /*feeds_attention: the attention step takes its own statistics*/) {
        T out = tensor(cout, x.H, x.W);
        const int mark = top, cin = x.C + (skip ? skip->C : 0);
        // Block = convolution with GroupNorm (+ FiLM) + SiLU in its epilogue (unet.py:57-73); block2 adds the residual there too
        T a1 = temp(cout, x.H, x.W);
        NormSpec n1{p + ".block1.norm", G, u->ss_off.at(p)}, n2{p + ".block2.norm", G, -1};
        flops += conv(x, skip, a1, p + ".block1.proj", 3, 1, 1, 0, 1, -1, 0, true, &n1);
        int res = x.off;
        if (cin != cout) {
            T rb = temp(cout, x.H, x.W);
            flops += conv(x, skip, rb, p + ".res_conv", 1, 0, 1, 0, 0, -1, 0);
            res = rb.off;
        }
        flops += conv(a1, nullptr, out, p + ".block2.proj", 3, 1, 1, 0, 1, res, 0, true, &n2);
        top = mark;
        return out;
    }
    T attention(const std::string& p, const T& x, bool full) {
        T out = tensor(x.C, x.H, x.W);
        const int mark = top, n = x.H * x.W;
        SStep s;
        s.op = full ? S_ATTN : S_LINATTN; s.in0 = x.off; s.out = out.off; s.C0 = x.C; s.Hi = x.H; s.Wi = x.W;
        if (n == 1) { s.op = S_ATTN1; s.full = full ? 1 : 0; }       // one position: the closed form (unet_sample.hip op_attention1)
        else if (!full && n <= 64 && (x.C == 8 || x.C == 16)) s.op = S_LINATTN_W;
        else if (!full && n <= 16 && x.C == 32) s.op = S_LINATTN_G;      // the same with its weights read from L2 (they do not fit the staging buffer)   // a wave per head (all four heads' weights fit the staging buffer: C * 512 floats)
        s.scratch = alloc(n == 1 ? 2 * x.C + 128 + SAMPLE_THREADS
                          : (s.op == S_LINATTN_W || s.op == S_LINATTN_G) ? 5 * n * x.C + 4 * (n + std::max(n, 32)) * 32
                          : 2 * n * x.C + 3 * n * 32 + (full ? n * n : 32 * 32) + n * 32);
        s.gamma = u->R(p + ".fn.norm.weight"); s.beta = u->R(p + ".fn.norm.bias");
        s.lc = ilog2(x.C); s.ln = ilog2(n);
        s.w = u->P(p + ".fn.fn.to_qkv.weight");
        if (full) { s.w2 = u->P(p + ".fn.fn.to_out.weight"); s.b2 = u->R(p + ".fn.fn.to_out.bias"); }
        else {
            s.w2 = u->P(p + ".fn.fn.to_out.0.weight"); s.b2 = u->R(p + ".fn.fn.to_out.0.bias");
            s.g2 = u->R(p + ".fn.fn.to_out.1.weight"); s.be2 = u->R(p + ".fn.fn.to_out.1.bias");
        }
        prog.push_back(s);
        flops += attn_flops(n, x.C, heads, full);
        top = mark;
        return out;
    }
    T stem() {
        xin = tensor(ch, H, W);
        if (u->cfg.mask_cond) mask = tensor(ch, H, W);
        T xi = tensor(dim, H, W);
        flops += conv(xin, nullptr, xi, "init_conv", 1, 0, 1, 0, 0, -1, 0);
        if (!u->cfg.mask_cond) return xi;
        T x0 = tensor(dim, H, W);                        // unet.py:298-305: replaces x when a mask is given that is not all ones
        const int mark = top;
        T f1 = temp(2 * dim, H, W), f2 = temp(2 * dim, H, W);
        conv(xi, &mask, f1, "mask_fusion_conv.0", 5, 2, 1, 0, 1, -1, 2);
        conv(f1, nullptr, f2, "mask_fusion_conv.2", 3, 1, 1, 0, 1, -1, 2);
        conv(f2, nullptr, x0, "mask_fusion_conv.4", 3, 1, 1, 0, 0, -1, 2);
        copy(xi, x0, 5);
        flops += 2.0 * H * W * (25.0 * (dim + ch) * 2 * dim + 9.0 * 2 * dim * 2 * dim + 9.0 * 2 * dim * dim);
        top = mark;
        retire(xi);
        return x0;
    }
    T inject(const std::string& name, const T& x) {       // x + SiLU(conv3x3(cat[x, bilinear(mask)])), unet.py:336-340,360-364
        T out = tensor(x.C, x.H, x.W);
        const int mark = top;
        T mr = temp(ch, x.H, x.W);
        SStep s;
        s.op = S_BILINEAR; s.guard = 1; s.in0 = mask.off; s.out = mr.off; s.C0 = ch; s.Hi = H; s.Wi = W; s.Ho = x.H; s.Wo = x.W;
        prog.push_back(s);
        flops += conv(x, &mr, out, name, 3, 1, 1, 0, 1, x.off, 1);
        copy(x, out, 3);
        top = mark;
        return out;
    }
    T downsample(const std::string& p, const T& x, int cout, bool last) {
        T o = last ? tensor(cout, x.H, x.W) : tensor(cout, x.H / 2, x.W / 2);
        flops += last ? conv(x, nullptr, o, p, 3, 1, 1, 0, 0, -1, 0) : conv(x, nullptr, o, p + ".1", 2, 0, 2, 0, 0, -1, 0);
        return o;
    }
    T upsample(const std::string& p, const T& x, int cout, bool last) {
        T o = last ? tensor(cout, x.H, x.W) : tensor(cout, x.H * 2, x.W * 2);
        flops += last ? conv(x, nullptr, o, p, 3, 1, 1, 0, 0, -1, 0) : conv(x, nullptr, o, p + ".1", 3, 1, 1, 1, 0, -1, 0);
        return o;
    }
    T head(const T& x, const T& x0) {
        T h = resblock("final_res_block", x, &x0, dim, false);
        T v = tensor(ch, H, W);
        flops += conv(h, nullptr, v, "final_conv", 1, 0, 1, 0, 0, -1, 0);
        return v;
    }
};

// Returns FC_OK and leaves ONE launch in the plan, or 1 when the model does not qualify (the caller then builds the ordinary plan).
static int build_sample_plan(fc_unet* u, Plan* pl, Builder& b, const WalkCfg& walk, int maxB, int H, int W) {
    // ON for the models that qualify unless FLOCODER_AMD_SAMPLE_KERNEL=0 (round 4, config 5's dim-8 / 4x8x8 flow: 538 us per evaluation
    // against 842 us for the 115 launches of the ordinary plan; profiles/r04_sample_kernel_stamps.txt).  A sample
    // is ONE workgroup, so the kernel's time is that of one sample as long as every sample has a CU of its own: beyond that the ordinary
    // plan (whose launches grow wider, not longer) wins again -- batches larger than the CU count keep it.
    static const bool off = [] { const char* e = std::getenv("FLOCODER_AMD_SAMPLE_KERNEL"); return e && std::string(e) == "0"; }();
    static const int cus = [] { int dev = 0, n = 0; if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 0; return n; }();
    if (maxB > cus) return 1;
    const fc_unet_config& c = u->cfg;
    if (off || u->keep_all || c.groups > 8 || u->heads != 4) return 1;
    SampleProgram e(u, H, W);
    const SampleProgram::T v = walk_unet(walk, e);
    const std::vector<SStep>& prog = e.prog;
    // every tensor at most four elements per thread, attention at most 64 channels / 64 keys (unet_sample.hip's register and staging budgets)
    // (powers of two throughout: the kernel indexes by shifts and masks)
    const int cap = 4 * SAMPLE_THREADS;
    for (const SStep& s : prog) {
        if (s.op == S_CONV && (s.Ho * s.Wo * s.Cout > cap || !is_pow2(s.Cout) || s.Cout < 4 || s.Cout > SAMPLE_THREADS || s.nchunk > 8 || (s.C0 & 3) || (s.C1 & 3) || s.C0 + s.C1 > 128)) return 1;     // (channel quads; the zero line is 128 floats)
        if (s.op == S_NORM && (s.Hi * s.Wi * s.C0 > cap || !is_pow2(s.C0) || s.C0 > 64 || !is_pow2(s.C0 / s.G) || s.G > 8)) return 1;
        if (s.op == S_CONV && s.fnorm && (s.Cout > 64 || !is_pow2(s.Cout / s.G) || s.G > 8)) return 1;
        if (s.op == S_LINATTN_W && ((s.C0 != 8 && s.C0 != 16) || !is_pow2(s.Hi * s.Wi) || s.Hi * s.Wi > 64)) return 1;
        if (s.op == S_LINATTN_G && (s.C0 != 32 || !is_pow2(s.Hi * s.Wi) || s.Hi * s.Wi > 16)) return 1;
        if (s.op == S_ATTN1 && (s.C0 > 64 || s.C0 < 8 || !is_pow2(s.C0))) return 1;
        if ((s.op == S_ATTN || s.op == S_LINATTN) && (s.C0 > 64 || s.C0 < 4 || !is_pow2(s.C0) || !is_pow2(s.Hi * s.Wi) || s.Hi * s.Wi * s.C0 > cap)) return 1;
        if (s.op == S_ATTN && s.Hi * s.Wi > 64) return 1;
    }
    e.top = e.peak;                                       // behind every temporary (they were released, not forgotten)
    const int zero_off = e.alloc(128);
    const int wbuf_off = e.alloc(2 * 4096), prog_off = e.alloc((int)(prog.size() * sizeof(SStep) / 4) + 4);
    const size_t lds = (size_t)e.peak * sizeof(float);
    if (lds > 158 * 1024) return 1;                       // the sample does not fit a CU: ordinary plan
    FC_TRY(unet_sample_init());
    SStep* dev = b.upload(prog);
    unsigned* done = reinterpret_cast<unsigned*>(b.dmalloc(4));
    if (b.err) return b.err;
    FC_HIP(hipMemset(done, 0, 4 * sizeof(unsigned)));
    SampleArgs a;
    a.prog = dev; a.nsteps = (int)prog.size(); a.S = u->S; a.ss = pl->ss; a.ch = c.channels; a.HW = H * W;
    a.x_off = e.xin.off; a.mask_off = e.mask.off; a.v_off = v.off; a.done = done; a.wbuf_off = wbuf_off; a.prog_off = prog_off; a.zero_off = zero_off;
    const bool mask_cond = c.mask_cond != 0;
    b.scope = "unet (one workgroup per sample)";
    b.push([a, lds, mask_cond](const FwdCtx& cx, hipStream_t s) {
        SampleArgs q = a;
        q.x = cx.x; q.x_mod = cx.x_mod; q.mask = mask_cond ? cx.mask : nullptr; q.mask_fuse = cx.mask_fuse;
        q.ss_all = cx.fetch.all; q.evalc = cx.fetch.all ? cx.fetch.evalc : nullptr; q.rows = cx.B; q.out = cx.out; q.euler = cx.euler;
        q.stamps = 5 * q.nsteps + 16 <= 4096 ? conv_stamp_buffer() : nullptr;   // (2 words per step + the phase split of the convolutions; fc_debug_set_conv_stamps: >= 4096 words)
        return unet_sample_launch(q, cx.B, lds, s);
    }, "unet_sample", e.flops);
    return FC_OK;
}

static int build_plan(fc_unet* u, Plan* pl, int maxB, int H, int W) {
    const fc_unet_config& c = u->cfg;
    const int L = c.n_levels, dim = c.dim, ch = c.channels;
    if (!is_pow2(H) || !is_pow2(W) || (H >> (L - 1)) < 1 || (W >> (L - 1)) < 1)
        return fail(FC_E_SHAPE, "unet: latent height/width must be powers of two >= 2^(levels-1)");
    if ((ch & 3) || (dim & 3)) return fail(FC_E_SHAPE, "unet: channels and dim must be multiples of 4");
    Builder b(u, pl, maxB, H, W);
    pl->flops = 0.0;
    pl->t_emb = b.dmalloc((size_t)maxB * u->td);
    pl->ss = b.dmalloc((size_t)maxB * u->S);
    const int td = u->td, S = u->S, ncls = c.n_classes;

    // -- conditioning (unet.py:310-316 and every ResnetBlock.mlp) --
    {
        TembArgs t;
        t.freqs = u->freqs;
        t.w1t = u->P("time_mlp.1.weight"); t.b1 = u->R("time_mlp.1.bias");
        t.w2t = u->P("time_mlp.3.weight"); t.b2 = u->R("time_mlp.3.bias");
        t.emb = t.cw1t = t.cb1 = t.cw2t = t.cb2 = nullptr;
        if (ncls > 0) {
            t.emb = u->R("class_cond_mlp.0.weight");
            t.cw1t = u->P("class_cond_mlp.1.weight"); t.cb1 = u->R("class_cond_mlp.1.bias");
            t.cw2t = u->P("class_cond_mlp.3.weight"); t.cb2 = u->R("class_cond_mlp.3.bias");
        }
        t.n_classes = ncls; t.t_out = pl->t_emb; t.dim = dim; t.td = td;
        u->temb_proto = t;
        b.scope = "time_mlp";
        float *hid = b.dmalloc((size_t)maxB * td), *chid = b.dmalloc((size_t)maxB * td);
        b.push([t, hid, chid](const FwdCtx& cx, hipStream_t s) {
            if (cx.fetch.all) return (int)FC_OK;   // this evaluation's rows were computed before the first step (fc_unet_integrate)
            TembArgs a = t; a.B = cx.B; a.time = cx.time; a.class_ids = cx.ids; a.class_batch_mod = cx.ids_mod; a.null_from = cx.null_from;
            return temb_launch(a, hid, chid, s);
        }, "temb", 2.0 * ((double)dim * td + (double)td * td * (ncls > 0 ? 3 : 1)));
        const float *te = pl->t_emb, *wt = u->P("__ss_wt"), *sb = u->P("__ss_bias");
        float* ss = pl->ss;
        b.scope = "resblock.mlp";
        b.push([=](const FwdCtx& cx, hipStream_t s) { return cx.fetch.all ? (int)FC_OK : ss_launch(te, wt, sb, ss, cx.B, td, S, s); }, "ss", 2.0 * (double)td * S);
    }

    WalkCfg walk;
    walk.n_levels = L; walk.mask_cond = c.mask_cond != 0; walk.cs = u->chans;
    // small models: the whole forward of a sample in one workgroup (unet_sample.hip); 1 = does not qualify
    const int r = build_sample_plan(u, pl, b, walk, maxB, H, W);
    if (r != FC_OK && r != 1) return r;
    if (r == 1) walk_unet(walk, b);
    if (b.err) return b.err;
    pl->maxB = maxB; pl->H = H; pl->W = W;
    return FC_OK;
}

// ---- process-wide guard of the meeting launches ------------------------------------------------------------------------------
// A launch whose workgroups wait for each other is only safe while no OTHER such launch can hold part of the CUs: two of them, each
// half resident, would wait for workgroups that cannot start (bounded by the spin limit, then NaN + error -- never a hang, never silent).
// Inside one process that cannot happen: a plan with meeting launches is ordered behind the previous one of ANY handle when that ran
// on another stream (one hipStreamWaitEvent, nothing when the event has completed).  Kernels without meetings beside it only delay it.
// Other processes on the same GPU are beyond this guard: that is what fc_unet_set_shared is for.
struct MeetGuard { std::mutex mu; hipEvent_t ev = nullptr; hipStream_t s = nullptr; const fc_unet* owner = nullptr; };
static MeetGuard g_meet[16];
static MeetGuard& meet_guard(int device) { return g_meet[device & 15]; }

static int plan_meets(const fc_unet* u) { return u->plan.n_meet; }

int meet_enter(fc_unet* u, hipStream_t s) {
    if (!plan_meets(u)) return FC_OK;
    MeetGuard& g = meet_guard(u->device);
    std::lock_guard<std::mutex> lk(g.mu);
    if (g.ev && g.s != s && hipEventQuery(g.ev) != hipSuccess) FC_HIP(hipStreamWaitEvent(s, g.ev, 0));
    return FC_OK;
}
int meet_leave(fc_unet* u, hipStream_t s) {
    if (!plan_meets(u)) return FC_OK;
    MeetGuard& g = meet_guard(u->device);
    std::lock_guard<std::mutex> lk(g.mu);
    FC_HIP(hipEventRecord(u->ev_meet, s));
    g.ev = u->ev_meet; g.s = s; g.owner = u;
    // the error word follows the work: the host sees it at its next synchronisation with `s` (fc_unet_check) or at the next call
    FC_HIP(hipMemcpyAsync(const_cast<int*>(u->host_err), u->dev_err, sizeof(int), hipMemcpyDeviceToHost, s));
    return FC_OK;
}
static void meet_forget(const fc_unet* u) {
    MeetGuard& g = meet_guard(u->device);
    std::lock_guard<std::mutex> lk(g.mu);
    if (g.owner == u) { g.ev = nullptr; g.s = nullptr; g.owner = nullptr; }
}
// refuse to go on after a timed-out meeting: the arena holds NaN-poisoned activations and whatever was returned since is invalid
int check_poison(fc_unet* u) {
    if (u->host_err && *u->host_err) u->tail_failed = true;
    if (u->tail_failed)
        return fail(FC_E_STATE, "unet: a fused Block tail timed out waiting for its sample group (the GPU was shared with other work while "
                                "the exclusive plan ran); the affected samples are NaN.  Rebuild the plan -- fc_unet_set_shared(handle, 1) "
                                "selects the plan without cross-workgroup waits");
    return FC_OK;
}

int check_ready(const fc_unet* u, int rows, int H, int W) {
    if (!u) return fail(FC_E_ARG, "null fc_unet");
    if (u->device < 0) return fail(FC_E_STATE, "unet: created with device < 0 (description only)");
    if (!u->loaded) return fail(FC_E_STATE, "unet: weights not loaded (fc_unet_load_params)");
    if (u->maxB < rows || u->H != H || u->W != W)
        return fail(FC_E_STATE, "unet: no plan for this shape; call fc_unet_reserve(rows >= " + std::to_string(rows) + ")");
    return FC_OK;
}

}  // namespace fc

// =============================================================================================== C ABI
extern "C" {

int fc_abi_version(void) { return FC_ABI_VERSION; }
const char* fc_last_error(void) { return fc::last_error(); }

int fc_check_device(int device) {
    hipDeviceProp_t prop;
    FC_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(FC_E_ARCH, std::string("flocoder_amd kernels are built for gfx950 only; device reports ") + prop.gcnArchName);
    return FC_OK;
}

int fc_unet_create(const fc_unet_config* cfg, int device, fc_unet** out) {
    if (!cfg || !out) return fail(FC_E_ARG, "fc_unet_create: null argument");
    if (cfg->n_levels < 1 || cfg->n_levels > 8 || cfg->dim < 4 || cfg->channels < 1 || cfg->groups < 1)
        return fail(FC_E_ARG, "fc_unet_create: bad config");
    for (int i = 0; i < cfg->n_levels; ++i)
        if (cfg->dim_mults[i] < 1 || !is_pow2(cfg->dim * cfg->dim_mults[i] / cfg->groups) || (cfg->dim * cfg->dim_mults[i]) % cfg->groups)
            return fail(FC_E_SHAPE, "fc_unet_create: channels per GroupNorm group must be a power of two");
    std::unique_ptr<fc_unet> u(new fc_unet);
    u->cfg = *cfg;
    u->device = device;
    u->want_k8 = true;
    FC_TRY(declare_all(u.get()));
    if (device < 0) {  // description only: parameter table without touching a GPU
        *out = u.release();
        return FC_OK;
    }
    FC_TRY(fc_check_device(device));
    FC_HIP(hipSetDevice(device));
    FC_TRY(conv_init());
    FC_TRY(linattn_fused_init());
    FC_TRY(linattn_sample_init());
    FC_TRY(temb_init());
    FC_TRY(u->alloc_device());
    const int half = cfg->dim / 2;
    std::vector<float> fr(half);
    const double lf = std::log(10000.0) / (half - 1);  // unet.py:26
    for (int k = 0; k < half; ++k) fr[k] = (float)std::exp((double)((float)k * (float)-lf));
    FC_HIP(hipMalloc(reinterpret_cast<void**>(&u->freqs), half * sizeof(float)));
    FC_HIP(hipMemcpy(u->freqs, fr.data(), half * sizeof(float), hipMemcpyHostToDevice));
    FC_HIP(hipStreamCreateWithFlags(&u->ig.stream, hipStreamNonBlocking));
    FC_HIP(hipEventCreateWithFlags(&u->ig.ev_in, hipEventDisableTiming));
    FC_HIP(hipEventCreateWithFlags(&u->ig.ev_out, hipEventDisableTiming));
    FC_HIP(hipEventCreateWithFlags(&u->ev_meet, hipEventDisableTiming));
    FC_HIP(hipMalloc(reinterpret_cast<void**>(&u->dev_err), sizeof(int)));
    FC_HIP(hipMemset(u->dev_err, 0, sizeof(int)));
    { void* hp = nullptr; FC_HIP(hipHostMalloc(&hp, sizeof(int), hipHostMallocDefault)); u->host_err = static_cast<volatile int*>(hp); *u->host_err = 0; }
    *out = u.release();
    return FC_OK;
}

void fc_unet_destroy(fc_unet* u) {
    if (!u) return;
    if (u->device < 0) { delete u; return; }
    (void)hipSetDevice(u->device);
    (void)hipDeviceSynchronize();
    free_plan(u);
    u->ig.release_handle();
    u->free_device();
    if (u->freqs) (void)hipFree(u->freqs);
    meet_forget(u);
    if (u->ev_meet) (void)hipEventDestroy(u->ev_meet);
    if (u->dev_err) (void)hipFree(u->dev_err);
    if (u->host_err) (void)hipHostFree(const_cast<int*>(u->host_err));
    delete u;
}

int fc_unet_param_count(const fc_unet* u) { return u ? (int)u->params.size() : 0; }

int fc_unet_param_info(const fc_unet* u, int i, const char** name, int64_t shape[4], int64_t* offset) {
    if (!u) return fail(FC_E_ARG, "fc_unet_param_info: null handle");
    return u->info(i, name, shape, offset);
}

int64_t fc_unet_param_numel(const fc_unet* u) { return u ? u->raw_numel : 0; }

int fc_unet_set_time_freqs(fc_unet* u, const float* freqs_host, int n) {
    if (!u || !freqs_host || n != u->cfg.dim / 2) return fail(FC_E_ARG, "fc_unet_set_time_freqs: expected dim/2 entries");
    FC_HIP(hipMemcpy(u->freqs, freqs_host, n * sizeof(float), hipMemcpyHostToDevice));
    return FC_OK;
}

int fc_unet_load_params(fc_unet* u, const float* flat, int64_t numel, int on_device, void* stream) {
    if (!u || !flat) return fail(FC_E_ARG, "fc_unet_load_params: null argument");
    if (u->device < 0) return fail(FC_E_STATE, "unet: created with device < 0 (description only)");
    FC_HIP(hipSetDevice(u->device));
    ++u->param_version;
    return u->load(flat, numel, on_device, static_cast<hipStream_t>(stream));
}

int fc_unet_reserved(const fc_unet* u, int* max_batch, int* height, int* width) {
    if (!u) return fail(FC_E_ARG, "fc_unet_reserved: null handle");
    if (max_batch) *max_batch = u->maxB;
    if (height) *height = u->maxB ? u->H : 0;
    if (width) *width = u->maxB ? u->W : 0;
    return FC_OK;
}

int fc_unet_reserve(fc_unet* u, int max_batch, int height, int width) {
    if (!u || max_batch < 1) return fail(FC_E_ARG, "fc_unet_reserve: bad argument");
    if (u->device < 0) return fail(FC_E_STATE, "unet: created with device < 0 (description only)");
    if (u->maxB >= max_batch && u->H == height && u->W == width) return FC_OK;
    FC_HIP(hipSetDevice(u->device));
    FC_HIP(hipDeviceSynchronize());
    free_plan(u);
    u->arena_touched(0);
    int r = build_plan(u, &u->plan, max_batch, height, width);
    if (r == FC_OK) r = alloc_integrator(u, max_batch, height, width);
    if (r != FC_OK) { free_plan(u); return r; }
    u->maxB = max_batch; u->H = height; u->W = width;
    return FC_OK;
}

int fc_unet_forward(fc_unet* u, const float* x, const float* time, const int64_t* ids, const float* mask, int mask_is_ones, float* out,
                    int B, int H, int W, void* stream) {
    FC_TRY(check_ready(u, B, H, W));
    if (!x || !time || !out || B < 1) return fail(FC_E_ARG, "fc_unet_forward: null argument");
    FwdCtx c;
    c.x = x; c.x_mod = B; c.time = time; c.ids = ids; c.ids_mod = B; c.null_from = 0;
    c.mask = u->cfg.mask_cond ? mask : nullptr;
    c.mask_fuse = (c.mask && !mask_is_ones) ? 1 : 0;
    c.out = out; c.B = B;
    FC_TRY(check_poison(u));
    u->arena_touched(u->keep_all ? B : 0);
    FC_TRY(meet_enter(u, static_cast<hipStream_t>(stream)));
    FC_TRY(run_plan(u->plan, c, static_cast<hipStream_t>(stream)));
    return meet_leave(u, static_cast<hipStream_t>(stream));
}

int fc_unet_set_shared(fc_unet* u, int shared) {
    if (!u) return fail(FC_E_ARG, "fc_unet_set_shared: null handle");
    if (u->device < 0) return fail(FC_E_STATE, "unet: created with device < 0 (description only)");
    if (u->shared == (shared != 0)) return FC_OK;
    u->shared = shared != 0;
    if (u->maxB > 0) {   // the plan in place was built for the other mode: drop it, the next reserve rebuilds
        FC_HIP(hipSetDevice(u->device));
        FC_HIP(hipDeviceSynchronize());
        const bool train = u->keep_all;
        free_plan(u);
        u->arena_touched(0);
        u->keep_all = train;
    }
    return FC_OK;
}

int fc_unet_meeting_launches(const fc_unet* u) { return u ? plan_meets(u) : 0; }

int fc_unet_check(fc_unet* u, void* stream, int synchronize) {
    if (!u) return fail(FC_E_ARG, "fc_unet_check: null handle");
    if (u->device < 0) return FC_OK;
    if (synchronize) {
        FC_HIP(hipSetDevice(u->device));
        FC_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    }
    return check_poison(u);
}

uint64_t fc_unet_arena_serial(const fc_unet* u) { return u ? u->arena_serial : 0; }

// Time every launch of the current plan on its own (profile_plan).
static int g_stamp_op = -1;                     // diagnostics: fc_unet_profile_ops runs this plan entry once more with the conv stamps on
static unsigned long long* g_stamp_op_buf = nullptr;
int fc_debug_set_stamp_op(int op_index, void* buf_dev) { g_stamp_op = buf_dev ? op_index : -1; g_stamp_op_buf = static_cast<unsigned long long*>(buf_dev); return FC_OK; }

int fc_unet_profile_ops(fc_unet* u, int batch, int repeats, float* ms_out, int n_out, void* stream) {
    if (!u || !ms_out || repeats < 1) return fail(FC_E_ARG, "fc_unet_profile_ops: bad argument");
    FC_TRY(check_ready(u, batch, u->H, u->W));
    const Plan& pl0 = u->plan;
    u->arena_touched(0);
    hipStream_t s = static_cast<hipStream_t>(stream);
    FwdCtx c;
    c.x = u->ig.y; c.x_mod = batch; c.time = u->ig.tvec; c.ids = nullptr; c.ids_mod = batch; c.out = u->ig.v2; c.B = batch;
    FC_HIP(hipMemsetAsync(u->ig.tvec, 0, batch * sizeof(float), s));
    auto stamp = [&](int i) -> int {            // the same launch once more, writing its in-kernel phase stamps
        if (i != g_stamp_op || !g_stamp_op_buf) return FC_OK;
        conv_set_stamp_buffer(g_stamp_op_buf);
        const int rc = pl0.ops[i](c, s);
        (void)hipStreamSynchronize(s);
        conv_set_stamp_buffer(nullptr);
        return rc;
    };
    return profile_plan(pl0, c, repeats, ms_out, n_out, s, stamp);
}

int fc_unet_op_info(const fc_unet* u, int i, const char** kernel, const char** module, double* flops_per_sample) {
    if (!u || i < 0 || i >= (int)u->plan.ops.size()) return fail(FC_E_ARG, "fc_unet_op_info: index out of range");
    if (kernel) *kernel = u->plan.op_kernel[i].c_str();
    if (module) *module = u->plan.op_what[i].c_str();
    if (flops_per_sample) *flops_per_sample = u->plan.op_flops[i];
    return FC_OK;
}

int fc_unet_op_bytes(const fc_unet* u, int i, double* bytes_per_sample, double* bytes_per_launch) {
    if (!u || i < 0 || i >= (int)u->plan.ops.size()) return fail(FC_E_ARG, "fc_unet_op_bytes: index out of range");
    if (bytes_per_sample) *bytes_per_sample = u->plan.op_bytes_ps[i];
    if (bytes_per_launch) *bytes_per_launch = u->plan.op_bytes_fixed[i];
    return FC_OK;
}

int fc_unet_chains(const fc_unet* u, int* rows_per_chain) {
    if (!u) return 0;
    if (rows_per_chain) *rows_per_chain = u->maxB;
    return 1;
}

int fc_unet_fused_tail_errors(const fc_unet* u, int* count) {
    if (!u || !count) return fail(FC_E_ARG, "fc_unet_fused_tail_errors: null argument");
    *count = 0;
    if (u->device < 0 || !u->dev_err) return FC_OK;
    int v = 0;
    FC_HIP(hipMemcpy(&v, u->dev_err, sizeof(int), hipMemcpyDeviceToHost));   // synchronises with the null stream; callers sync their own
    *count = (v != 0 || u->tail_failed) ? 1 : 0;
    return FC_OK;
}

int fc_unet_plan_launches(const fc_unet* u) { return u ? (int)u->plan.ops.size() : 0; }
double fc_unet_flops_per_sample(const fc_unet* u) { return u ? u->plan.flops : 0.0; }

// fc_unet_train_reserve switches a handle to plans that keep every intermediate, for good.  A caller that needed the backward plan for
// one call only (Unet.log_likelihood on a model that otherwise samples) asks which form the handle is in and puts the inference form back:
// the plans are dropped and the next fc_unet_reserve builds the inference plan a handle that never trained would build.  Synchronises.
int fc_unet_train_form(const fc_unet* u) { return (u && u->keep_all) ? 1 : 0; }

int fc_unet_train_release(fc_unet* u) {
    if (!u) return fail(FC_E_ARG, "fc_unet_train_release: null handle");
    if (u->device < 0 || !u->keep_all) return FC_OK;
    FC_HIP(hipSetDevice(u->device));
    FC_HIP(hipDeviceSynchronize());
    free_plan(u);
    u->keep_all = false;
    u->arena_touched(0);
    return FC_OK;
}

// ---- debug / test hooks --------------------------------------------------------------------------
int fc_unet_debug_tensor(const fc_unet* u, const char* name, const float** ptr, int* C, int* H, int* W) {
    if (!u || !name) return fail(FC_E_ARG, "fc_unet_debug_tensor: null argument");
    auto it = u->plan.named.find(name);
    if (it == u->plan.named.end()) {
        it = u->bwd.named.find(name);        // "grad:<tap>": gradient of that tap after fc_unet_backward
        if (it == u->bwd.named.end()) return fail(FC_E_ARG, std::string("fc_unet_debug_tensor: no tap named ") + name);
    }
    *ptr = it->second.p; *C = it->second.C; *H = it->second.H; *W = it->second.W;
    return FC_OK;
}

// Test hook: put the arrival counter of one meeting launch out of step, so that its workgroups draw different epochs and every wait of
// that launch times out (bounded spins) -- the failure a shared device can cause, on demand.
int fc_debug_unet_break_meeting(fc_unet* u) {
    if (!u || u->plan.fin_sync.empty()) return fail(FC_E_STATE, "fc_debug_unet_break_meeting: the plan has no meeting launch");
    FC_HIP(hipDeviceSynchronize());
    unsigned v = 0;
    FC_HIP(hipMemcpy(&v, u->plan.fin_sync[0], sizeof(unsigned), hipMemcpyDeviceToHost));
    ++v;
    FC_HIP(hipMemcpy(u->plan.fin_sync[0], &v, sizeof(unsigned), hipMemcpyHostToDevice));
    return FC_OK;
}

int fc_debug_unet_break_meeting_kind(fc_unet* u, int kind) {      // the same for the first meeting launch of a kind (0 Block tail, 1 linear attention close)
    if (!u) return fail(FC_E_ARG, "fc_debug_unet_break_meeting_kind: null handle");
    const Plan& pl = u->plan;
    for (size_t i = 0; i < pl.fin_sync.size(); ++i)
        if (pl.fin_kind[i] == kind) {
            FC_HIP(hipDeviceSynchronize());
            unsigned v = 0;
            FC_HIP(hipMemcpy(&v, pl.fin_sync[i], sizeof(unsigned), hipMemcpyDeviceToHost));
            ++v;
            FC_HIP(hipMemcpy(pl.fin_sync[i], &v, sizeof(unsigned), hipMemcpyHostToDevice));
            return FC_OK;
        }
    return fail(FC_E_STATE, "fc_debug_unet_break_meeting_kind: the plan has no meeting launch of that kind");
}

int fc_debug_set_fused_tail(int on) {   // plans built from now on use (1) / do not use (0) the meeting launches; < 0: back to the default (on)
    fc::g_fused_tail = on < 0 ? -1 : (on ? 1 : 0);
    return FC_OK;
}

// Diagnostics: record which instantiation of the pipelined convolution every launch goes to (on != 0 starts an empty record, 0 stops);
// fc_debug_conv_routes_read copies the record -- one line of the thirteen template arguments per launch -- and returns its length.
int fc_debug_conv_routes(int on) { conv_route_log_set(on != 0); linattn_route_log_set(on != 0); step_route_log_set(on != 0); return FC_OK; }
int fc_debug_step_routes_read(char* buf, int cap) {
    const std::string r = step_route_log_get();
    if (buf && cap > 0) { const size_t n = r.size() < (size_t)cap - 1 ? r.size() : (size_t)cap - 1; memcpy(buf, r.data(), n); buf[n] = 0; }
    return (int)r.size();
}
int fc_debug_conv_routes_read(char* buf, int cap) {
    const std::string r = conv_route_log_get();
    if (buf && cap > 0) { const size_t n = r.size() < (size_t)cap - 1 ? r.size() : (size_t)cap - 1; memcpy(buf, r.data(), n); buf[n] = 0; }
    return (int)r.size();
}

// Diagnostics: the table of conv_pipe_kernel instantiations (conv_pipe.hip build_rows), one line of the thirteen template arguments per row.
// Host code only: works before conv_init() and without a device.
int fc_debug_conv_table_read(char* buf, int cap) {
    const std::string r = conv_table_list();
    if (buf && cap > 0) { const size_t n = r.size() < (size_t)cap - 1 ? r.size() : (size_t)cap - 1; memcpy(buf, r.data(), n); buf[n] = 0; }
    return (int)r.size();
}

int fc_debug_linattn_routes_read(char* buf, int cap) {
    const std::string r = linattn_route_log_get();
    if (buf && cap > 0) { const size_t n = r.size() < (size_t)cap - 1 ? r.size() : (size_t)cap - 1; memcpy(buf, r.data(), n); buf[n] = 0; }
    return (int)r.size();
}

int fc_debug_set_conv_stamps(void* buf_dev) {
    conv_set_stamp_buffer(static_cast<unsigned long long*>(buf_dev));
    return FC_OK;
}

int fc_debug_copy(void* dst_dev, const void* src_dev, int64_t bytes, void* stream) {
    FC_HIP(hipMemcpyAsync(dst_dev, src_dev, (size_t)bytes, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return FC_OK;
}

static int g_debug_conv_prec = 0;
int fc_debug_set_conv_precision(int mode) { g_debug_conv_prec = mode == 1 ? 1 : 0; return FC_OK; }   // arithmetic of fc_debug_conv launches (tests)

int fc_debug_conv(const float* src0, int c0, const float* src1, int c1, const float* w_oihw, const float* bias, const float* add,
                  float* out, float* stats_out, int groups_out, int* stats_T, float* stats_nt, int batch, int hs, int ws, int cout,
                  int ksize, int pad, int stride, int upsample, int out_act, int tile_cfg, int repeats, float* ms_out, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    FC_TRY(conv_init());
    ConvArgs a;
    a.s0.p = src0; a.s0.C = c0; a.s1.p = src1; a.s1.C = src1 ? c1 : 0;
    a.Cin = a.s0.C + a.s1.C; a.Cout = cout; a.B = batch; a.Hs = hs; a.Ws = ws;
    a.KS = ksize; a.pad = pad; a.stride = stride; a.ups = upsample;
    a.H = upsample ? hs * 2 : (hs + 2 * pad - ksize) / stride + 1;
    a.W = upsample ? ws * 2 : (ws + 2 * pad - ksize) / stride + 1;
    a.bias = bias; a.add = add; a.out = out; a.out_act = out_act;
    a.stats_out = stats_out; a.Gout = groups_out;
    a.prec = g_debug_conv_prec;
    // the weights as a plan would carry them, packed by the plans' own packer: one buffer, one transient table of one to three jobs
    const int KK = ksize * ksize, ipad = (a.Cin + 15) / 16 * 16;
    const bool k8 = ksize == 3 && a.Cin % 32 == 0 && cout % 32 == 0;    // the k-step-quad copy where the shapes allow it (conv_pipe.hip FL_W4)
    const bool b3 = a.prec == 1 && ksize >= 1 && ksize <= 3;            // the split-bf16 copy when that arithmetic is asked for (the kernel sizes of conv_bf3_form)
    const size_t n = ((size_t)cout * a.Cin * KK + 63) & ~(size_t)63, n3 = (size_t)cout * ipad * KK;    // each copy 256-byte aligned
    float* wp = nullptr;
    FC_HIP(hipMalloc(reinterpret_cast<void**>(&wp), (n + (k8 ? n : 0) + (b3 ? n3 : 0)) * sizeof(float)));
    float* const wp8 = wp + n;
    float* const wp3 = wp8 + (k8 ? n : 0);
    std::vector<PackJob> jobs{pack_job_conv(cout, a.Cin, KK).at(w_oihw, wp)};
    a.w = wp;
    if (k8) { a.w4 = wp8; jobs.push_back(pack_job_conv_k8(cout, a.Cin, KK).at(w_oihw, wp8)); }
    if (b3) { a.w_b3 = wp3; jobs.push_back(pack_job_conv_b3(cout, a.Cin, KK, ipad).at(w_oihw, wp3)); }
    PackTable table;
    int r = pack_table_build(jobs, &table);
    if (r == FC_OK) r = pack_table_launch(table, s);
    ConvGeom g;
    if (r == FC_OK) r = conv_plan(a, tile_cfg, &g);
    if (r == FC_OK) { if (stats_T) *stats_T = g.T; if (stats_nt) *stats_nt = g.n_t; r = conv_launch(a, g.tile, s); }
    if (r == FC_OK && repeats > 0 && ms_out) {   // back-to-back timing of the same launch (warm caches)
        hipEvent_t e0, e1;
        (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
        (void)hipEventRecord(e0, s);
        for (int i = 0; i < repeats && r == FC_OK; ++i) r = conv_launch(a, g.tile, s);
        (void)hipEventRecord(e1, s);
        (void)hipEventSynchronize(e1);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        *ms_out = ms / repeats;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    }
    (void)hipStreamSynchronize(s);
    table.release();
    (void)hipFree(wp);
    return r;
}

// Tests: `n` weight re-layout jobs as ONE table launch on `stream`.  kinds[i] is a PackKind, dims + 5 * i the arguments of its constructor
// in order (the rest zero); dst_floats[i] (when not null) receives the size of job i's destination in floats; with src or dst null nothing runs.
int fc_debug_pack(int n, const int* kinds, const int* dims, const float* const* src, float* const* dst, int64_t* dst_floats, void* stream) {
    if (n < 0 || !kinds || !dims) return fail(FC_E_ARG, "fc_debug_pack: null argument");
    std::vector<PackJob> jobs;
    for (int i = 0; i < n; ++i) {
        const int* d = dims + 5 * i;
        PackJob j;
        switch (kinds[i]) {
            case PACK_CONV: j = pack_job_conv(d[0], d[1], d[2]); break;
            case PACK_S2D: j = pack_job_s2d(d[0], d[1]); break;
            case PACK_TRANSPOSE: j = pack_job_transpose(d[0], d[1], d[2], d[3]); break;
            case PACK_COPY: j = pack_job_copy(d[0]); break;
            case PACK_CONV_PAD: j = pack_job_conv_pad(d[0], d[1], d[2], d[3], d[4]); break;
            case PACK_DGRAD: j = pack_job_dgrad(d[0], d[1], d[2], d[3], d[4]); break;
            case PACK_CONV_K8: j = pack_job_conv_k8(d[0], d[1], d[2]); break;
            case PACK_CONV_B3: j = pack_job_conv_b3(d[0], d[1], d[2], d[3]); break;
            case PACK_UP4: j = pack_job_up4(d[0], d[1]); break;
            case PACK_UP4_B3: j = pack_job_up4_b3(d[0], d[1], d[2]); break;
            default: j = pack_spec((PackKind)kinds[i], 0, d[0], d[1], d[2], d[3], d[4]); break;      // for pack_table_build to refuse
        }
        if (dst_floats) dst_floats[i] = j.kind == PACK_TRANSPOSE ? (int64_t)j.b * j.c : (int64_t)j.total;   // the split layouts: two 16-bit parts of `total`
        jobs.push_back(j.at(src ? src[i] : nullptr, dst ? dst[i] : nullptr));
    }
    PackTable table;
    int r = pack_table_build(jobs, &table);
    if (r == FC_OK && src && dst) r = pack_table_launch(table, static_cast<hipStream_t>(stream));
    (void)hipStreamSynchronize(static_cast<hipStream_t>(stream));     // the table's device memory goes with this call
    table.release();
    return r;
}

int fc_debug_conv_wgrad(const float* src0, int c0, const float* src1, int c1, const float* dy, int cout, int batch, int hs, int ws, int ksize,
                        int pad, int stride, int upsample, float* dw_out, float* db_out, void* stream) {
    return fc_debug_conv_wgrad_ex(src0, c0, src1, c1, dy, cout, batch, hs, ws, ksize, pad, stride, upsample, dw_out, db_out, 0, 0, nullptr, nullptr,
                                  nullptr, stream);
}

int fc_debug_conv_wgrad_ex(const float* src0, int c0, const float* src1, int c1, const float* dy, int cout, int batch, int hs, int ws, int ksize,
                           int pad, int stride, int upsample, float* dw_out, float* db_out, int split_target, int accumulate, int* nsplit_out,
                           int* mtiles_out, int* tb_out, void* stream) {
    if (split_target < 0) return fail(FC_E_ARG, "fc_debug_conv_wgrad_ex: split_target must not be negative");
    hipStream_t s = static_cast<hipStream_t>(stream);
    FC_TRY(conv_wgrad_init());
    WgradArgs a;
    a.x0 = src0; a.C0 = c0; a.x1 = src1; a.C1 = src1 ? c1 : 0; a.Cin = a.C0 + a.C1; a.Cout = cout; a.dy = dy;
    a.B = batch; a.Hs = hs; a.Ws = ws; a.KS = ksize; a.pad = pad; a.stride = stride; a.ups = upsample;
    a.H = upsample ? hs * 2 : (hs + 2 * pad - ksize) / stride + 1;
    a.W = upsample ? ws * 2 : (ws + 2 * pad - ksize) / stride + 1;
    a.dw = dw_out; a.db = db_out;
    if (split_target > 0) a.split_target = split_target;
    const size_t need = conv_wgrad_workspace(a);
    float* wsp = nullptr;
    if (need) FC_HIP(hipMalloc(reinterpret_cast<void**>(&wsp), need * sizeof(float)));
    a.ws = wsp; a.ws_floats = need;
    int r = conv_wgrad_tiling(a, nsplit_out, mtiles_out, tb_out);
    if (r == FC_OK) r = conv_wgrad_launch(a, s, accumulate != 0);
    (void)hipStreamSynchronize(s);
    if (wsp) (void)hipFree(wsp);
    return r;
}

int fc_ot_pairing(const float* source_dev, const float* target_dev, int batch, int64_t dim, float* dist_ws_dev, int64_t* perm_out_dev,
                  void* stream) {
    if (!source_dev || !target_dev || !dist_ws_dev || !perm_out_dev) return fail(FC_E_ARG, "fc_ot_pairing: null argument");
    return ot_launch(source_dev, target_dev, batch, dim, dist_ws_dev, perm_out_dev, static_cast<hipStream_t>(stream));
}

int fc_ot_pairing_exact(const float* source_dev, const float* target_dev, int batch, int64_t dim, float* cost_ws_dev, int64_t* perm_out_dev,
                        double* duals_out_dev, void* stream) {
    if (batch < 1 || batch > 1024) return fail(FC_E_SHAPE, "fc_ot_pairing_exact: batch must be in [1, 1024]");   // before the null test: an empty batch has no pointers
    if (!source_dev || !target_dev || !cost_ws_dev || !perm_out_dev) return fail(FC_E_ARG, "fc_ot_pairing_exact: null argument");
    return ot_exact_launch(source_dev, target_dev, batch, dim, cost_ws_dev, perm_out_dev, duals_out_dev, static_cast<hipStream_t>(stream));
}

int fc_ot_assign(const float* cost_dev, int batch, int64_t* perm_out_dev, double* duals_out_dev, void* stream) {
    if (batch < 1 || batch > 1024) return fail(FC_E_SHAPE, "fc_ot_assign: batch must be in [1, 1024]");
    if (!cost_dev || !perm_out_dev) return fail(FC_E_ARG, "fc_ot_assign: null argument");
    return ot_assign_launch(cost_dev, batch, perm_out_dev, duals_out_dev, static_cast<hipStream_t>(stream));
}

int fc_ot_sinkhorn(const float* cost_dev, int batch, double reg, int max_iter, double stop_thr, float* plan_out_dev, double* duals_out_dev,
                   double* info_out_dev, void* stream) {
    if (batch < 1 || batch > 1024) return fail(FC_E_SHAPE, "fc_ot_sinkhorn: batch must be in [1, 1024]");
    if (!cost_dev || !plan_out_dev || !duals_out_dev || !info_out_dev) return fail(FC_E_ARG, "fc_ot_sinkhorn: null argument");
    return ot_sinkhorn_launch(cost_dev, batch, reg, max_iter, stop_thr, plan_out_dev, duals_out_dev, info_out_dev, static_cast<hipStream_t>(stream));
}

int fc_ot_plan_sinkhorn(const float* source_dev, const float* target_dev, int batch, int64_t dim, double reg, int normalize_cost, int max_iter,
                        double stop_thr, float* plan_out_dev, double* duals_out_dev, double* info_out_dev, float* cost_ws_dev, void* stream) {
    if (batch < 1 || batch > 1024) return fail(FC_E_SHAPE, "fc_ot_plan_sinkhorn: batch must be in [1, 1024]");
    if (dim < 1) return fail(FC_E_SHAPE, "fc_ot_plan_sinkhorn: dim must be positive");
    if (!source_dev || !target_dev || !plan_out_dev || !duals_out_dev || !info_out_dev || !cost_ws_dev)
        return fail(FC_E_ARG, "fc_ot_plan_sinkhorn: null argument");
    if (!(reg > 0.0) || !(stop_thr >= 0.0) || max_iter < 1 || max_iter > 10000)      // before anything is launched
        return fail(FC_E_ARG, "fc_ot_plan_sinkhorn: reg must be positive, stop_thr >= 0 and max_iter in [1, 10000]");
    hipStream_t s = static_cast<hipStream_t>(stream);
    FC_TRY(ot_sqdist_launch(source_dev, target_dev, batch, dim, cost_ws_dev, s));
    if (normalize_cost) FC_TRY(ot_normalize_launch(cost_ws_dev, batch, s));
    return ot_sinkhorn_launch(cost_ws_dev, batch, reg, max_iter, stop_thr, plan_out_dev, duals_out_dev, info_out_dev, s);
}

int fc_ot_sample_plan(const float* plan_dev, int batch, int n_pairs, uint64_t seed, uint32_t draw_index, int64_t* i_out_dev, int64_t* j_out_dev,
                      int* info_dev, void* stream) {
    if (batch < 1 || batch > 1024) return fail(FC_E_SHAPE, "fc_ot_sample_plan: batch must be in [1, 1024]");
    if (n_pairs < 1 || n_pairs > 65536) return fail(FC_E_SHAPE, "fc_ot_sample_plan: n_pairs must be in [1, 65536]");
    if (!plan_dev || !i_out_dev || !j_out_dev) return fail(FC_E_ARG, "fc_ot_sample_plan: null argument");
    return ot_sample_plan_launch(plan_dev, batch, n_pairs, seed, draw_index, i_out_dev, j_out_dev, info_dev, static_cast<hipStream_t>(stream));
}

int fc_ot_plan_pairing(const float* plan_dev, int batch, int64_t* perm_out_dev, void* stream) {
    if (batch < 1 || batch > 1024) return fail(FC_E_SHAPE, "fc_ot_plan_pairing: batch must be in [1, 1024]");
    if (!plan_dev || !perm_out_dev) return fail(FC_E_ARG, "fc_ot_plan_pairing: null argument");
    return ot_sweep_largest_launch(plan_dev, batch, perm_out_dev, static_cast<hipStream_t>(stream));
}

}  // extern "C"
