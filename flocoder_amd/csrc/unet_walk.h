// The velocity U-Net's topology in execution order (Unet._forward, unet.py:326-372), written once for both forward plan builders of
// unet.hip: the ordinary launch plan and the one-workgroup-per-sample LDS program.  The walk owns the skip stack, the module names and the
// liveness protocol; an emitter E turns each step into launches or program steps over its tensor type E::T:
//   stem() -> x0                                      init_conv (+ mask fusion)
//   resblock(p, x, skip, cout, feeds_attention)       ResnetBlock on cat[x, *skip] (skip may be null); feeds_attention: attention is next
//   attention(p, x, full)                             Residual(PreNorm(LinearAttention)), or the full softmax form
//   inject(name, x)                                   x + SiLU(conv3x3(cat[x, bilinear(mask)]))
//   downsample / upsample(p, x, cout, last)           last: the 3x3 convolution that keeps the resolution
//   head(x, x0)                                       final_res_block on cat[x, x0], then final_conv
//   retire(t)                                         the last reader of t has been emitted
// Every tensor a step reads or writes is alive for the whole step: the new tensor is taken first, the old one retired after.
#pragma once
#include <string>
#include <vector>

namespace fc {

struct WalkCfg {
    int n_levels = 0;
    bool mask_cond = false;
    std::vector<int> cs;      // [dim, dim * mult[0], dim * mult[1], ...]: level i maps cs[i] -> cs[i + 1] channels
};

template <class E> typename E::T walk_unet(const WalkCfg& c, E& e) {
    using T = typename E::T;
    const int L = c.n_levels;
    const std::vector<int>& cs = c.cs;
    auto injects = [&](int i) { return c.mask_cond && i < 2 && i < L; };      // {down,up}_mask_fusions hold min(2, L) layers (unet.py:224-235)
    std::vector<T> skips;
    const T x0 = e.stem();
    T x = x0;
    bool held = true;         // someone later reads x (it is x0, which head reads, or on the skip stack): advancing leaves it alive
    auto advance = [&](const T& y) { if (!held) e.retire(x); x = y; held = false; };
    auto push_skip = [&] { skips.push_back(x); held = true; };
    for (int i = 0; i < L; ++i) {                                              // unet.py:326-343
        const std::string p = "downs." + std::to_string(i);
        advance(e.resblock(p + ".0", x, nullptr, cs[i], false));
        push_skip();
        advance(e.resblock(p + ".1", x, nullptr, cs[i], true));
        advance(e.attention(p + ".2", x, false));
        push_skip();
        if (injects(i)) advance(e.inject("down_mask_fusions." + std::to_string(i) + ".0", x));
        advance(e.downsample(p + ".3", x, cs[i + 1], i == L - 1));
    }
    advance(e.resblock("mid_block1", x, nullptr, cs[L], true));                // unet.py:345-347
    advance(e.attention("mid_attn", x, true));
    advance(e.resblock("mid_block2", x, nullptr, cs[L], false));
    for (int i = 0; i < L; ++i) {                                              // unet.py:350-367, (dim_in, dim_out) = reversed(in_out)[i]
        const std::string p = "ups." + std::to_string(i);
        const int din = cs[L - 1 - i], dout = cs[L - i];
        for (int j = 0; j < 2; ++j) {
            const T s = skips.back();
            skips.pop_back();
            advance(e.resblock(p + (j ? ".1" : ".0"), x, &s, dout, j == 1));
            e.retire(s);
        }
        advance(e.attention(p + ".2", x, false));
        if (injects(i)) advance(e.inject("up_mask_fusions." + std::to_string(i) + ".0", x));
        advance(e.upsample(p + ".3", x, din, i == L - 1));
    }
    const T v = e.head(x, x0);                                                 // unet.py:369-372
    e.retire(x);
    e.retire(x0);
    return v;
}

}  // namespace fc
