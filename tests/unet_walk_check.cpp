// The liveness protocol and the module order of walk_unet (csrc/unet_walk.h), driven with a recording emitter: no GPU, no HIP header.
// Built and run by tests/test_unet_walk_cpu.py under AddressSanitizer and UBSan; exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "unet_walk.h"

static int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failed; std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

struct Recorder {
    using T = int;                                  // a tensor is its index into `retired`
    std::string tag;                                // the configuration, for messages
    std::vector<int> retired;                       // times tensor i was retired
    std::vector<std::string> names, made_by;        // module names in call order; what made tensor i
    std::vector<T> skips_read;                      // the skip argument of every resblock that had one, in call order
    std::vector<T> after_0, after_2;                // outputs of downs.i.0 and downs.i.2: what unet.py appends to h

    T make(const std::string& by) { retired.push_back(0); made_by.push_back(by); return (T)retired.size() - 1; }
    void live(T t, const std::string& at) {
        CHECK(t >= 0 && t < (T)retired.size(), "%s: %s reads an unknown tensor %d", tag.c_str(), at.c_str(), t);
        if (t >= 0 && t < (T)retired.size()) CHECK(retired[t] == 0, "%s: %s reads tensor %d (made by %s) after it was retired", tag.c_str(), at.c_str(), t, made_by[t].c_str());
    }
    T step(const std::string& name, T x, const T* second = nullptr) {
        live(x, name);
        if (second) live(*second, name);
        names.push_back(name);
        return make(name);
    }

    T stem() { return make("stem"); }
    T resblock(const std::string& p, T x, const T* skip, int, bool) {
        if (skip) skips_read.push_back(*skip);
        const T out = step(p, x, skip);
        if (p.compare(0, 6, "downs.") == 0 && p.back() == '0') after_0.push_back(out);
        return out;
    }
    T attention(const std::string& p, T x, bool) {
        const T out = step(p, x);
        if (p.compare(0, 6, "downs.") == 0) after_2.push_back(out);
        return out;
    }
    T inject(const std::string& name, T x) { return step(name, x); }
    T downsample(const std::string& p, T x, int, bool) { return step(p, x); }
    T upsample(const std::string& p, T x, int, bool) { return step(p, x); }
    T head(T x, T x0) {
        const T h = step("final_res_block", x, &x0);
        return step("final_conv", h);               // (h is the emitter's own: the walk never sees it)
    }
    void retire(T t) {
        live(t, "retire");
        if (t >= 0 && t < (T)retired.size()) ++retired[t];
    }
};

// Unet._forward (unet.py:326-372) for dim_mults of four levels with mask conditioning, module by module
static const char* const kForwardL4Mask[] = {
    "downs.0.0", "downs.0.1", "downs.0.2", "down_mask_fusions.0.0", "downs.0.3",
    "downs.1.0", "downs.1.1", "downs.1.2", "down_mask_fusions.1.0", "downs.1.3",
    "downs.2.0", "downs.2.1", "downs.2.2", "downs.2.3",
    "downs.3.0", "downs.3.1", "downs.3.2", "downs.3.3",
    "mid_block1", "mid_attn", "mid_block2",
    "ups.0.0", "ups.0.1", "ups.0.2", "up_mask_fusions.0.0", "ups.0.3",
    "ups.1.0", "ups.1.1", "ups.1.2", "up_mask_fusions.1.0", "ups.1.3",
    "ups.2.0", "ups.2.1", "ups.2.2", "ups.2.3",
    "ups.3.0", "ups.3.1", "ups.3.2", "ups.3.3",
    "final_res_block", "final_conv"};

int main() {
    for (int L = 1; L <= 4; ++L)
        for (int mask = 0; mask < 2; ++mask) {
            fc::WalkCfg c;
            c.n_levels = L; c.mask_cond = mask != 0;
            for (int i = 0; i <= L; ++i) c.cs.push_back(8 << i);
            Recorder r;
            r.tag = "L=" + std::to_string(L) + (mask ? " mask" : "");
            const int out = fc::walk_unet(c, r);
            const int h = out - 1;                  // final_res_block's output, made and kept by the emitter's head
            for (int t = 0; t < (int)r.retired.size(); ++t) {
                CHECK(r.retired[t] <= 1, "%s: tensor %d (made by %s) retired %d times", r.tag.c_str(), t, r.made_by[t].c_str(), r.retired[t]);
                if (t != out && t != h) CHECK(r.retired[t] == 1, "%s: tensor %d (made by %s) is still alive at return", r.tag.c_str(), t, r.made_by[t].c_str());
            }
            CHECK(r.retired[out] == 0, "%s: the returned tensor was retired", r.tag.c_str());
            // the skip stack: unet.py appends after block1 and after attn, the up path pops from the end -- and nothing is left on it
            std::vector<int> want;
            for (int i = L - 1; i >= 0; --i) { want.push_back(r.after_2[i]); want.push_back(r.after_0[i]); }
            CHECK(r.skips_read == want, "%s: skips are not popped in the reverse of the order they were pushed", r.tag.c_str());
            const int inj = mask ? (L < 2 ? L : 2) : 0;
            CHECK((int)r.names.size() == 8 * L + 5 + 2 * inj, "%s: %d modules", r.tag.c_str(), (int)r.names.size());
            if (L == 4 && mask) {
                const std::vector<std::string> ref(std::begin(kForwardL4Mask), std::end(kForwardL4Mask));
                CHECK(r.names == ref, "%s: module order differs from unet.py's forward", r.tag.c_str());
                for (size_t i = 0; i < r.names.size() && i < ref.size(); ++i)
                    if (r.names[i] != ref[i]) { std::printf("  first difference at %zu: %s, expected %s\n", i, r.names[i].c_str(), ref[i].c_str()); break; }
            }
        }
    if (g_failed) { std::printf("%d checks failed\n", g_failed); return 1; }
    std::printf("unet_walk_check: ok\n");
    return 0;
}
