// Generic pieces of the native runtimes (unet.hip, vae.hip): parameter store with the reference's state_dict names, weight
// packing, launch plan over a fixed activation arena, and the builder that emits implicit-GEMM launches.
#pragma once
#include <cmath>
#include <functional>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"

namespace fc {

struct Param {
    std::string name;
    int64_t shape[4] = {0, 0, 0, 0};
    int64_t numel = 0, offset = 0;
};

struct Act { float* p = nullptr; int C = 0, H = 0, W = 0; };
struct Stat { float* p = nullptr; int G = 0, T = 0; float n_t = 0.f; };

struct FwdCtx {             // per-call inputs of one forward
    const float* x = nullptr;          // NCHW [x_mod][C][H][W]
    int x_mod = 0;                     // row b reads sample b % x_mod (CFG: both halves share x)
    const float* time = nullptr;       // [B]
    const int64_t* ids = nullptr;      // [ids_mod] or null
    int ids_mod = 0, null_from = 0;
    const float* mask = nullptr;       // NCHW [x_mod][C][H][W] or null
    int mask_fuse = 0;                 // run mask_fusion_conv (mask present and not all ones)
    float* out = nullptr;              // NCHW [B][C][H][W]
    int B = 0;
    const float* d_out = nullptr;      // backward only: NCHW gradient of `out`
    float* grads = nullptr;            // backward only: flat parameter gradients, table layout
    bool grads_acc = false;            // backward only: add to `grads` instead of replacing its contents (fc_unet_backward_accumulate)
    float* dx_out = nullptr;           // backward only, optional: NCHW gradient of the input x
    float* dmask_out = nullptr;        // backward only, optional: NCHW gradient of the mask
    EulerTail euler;                   // integrator only: the Euler update rides in final_conv
    CondFetch fetch;                   // integrator only: conditioning rows of every evaluation were computed up front
    const StepClose* step = nullptr;   // integrator only: final_res_block's closing launch closes the Euler step as well (conv_dev.h FL_STEP) --
                                       // the init_conv and final_conv entries launch nothing, `euler` / `fetch` travel in the device block
};
using Op = std::function<int(const FwdCtx&, hipStream_t)>;

// What the backward pass needs to know about the forward's modules: the raw tensors and statistics each one left in the arena.
struct ResRec { std::string p; Act x, skip, h1, h2, rb, out; Stat st1, st2; int cout = 0; };
struct LinRec { std::string p; Act x, qkv, lao, yb, out; float* ctx = nullptr; Stat gn1, sty; };
struct MidRec { Act x, qkv, ao, out; Stat gn1; };
struct ConvRec { std::string name; Act x, out; int KS = 1, pad = 0, stride = 1, ups = 0; };
struct InjRec { std::string name; Act x, mr, z, out; };                      // x + SiLU(conv3x3(cat[x, bilinear(mask)])), unet.py:336-340
struct FuseRec { bool present = false; Act xi, mask, z1, f1, z2, f2, x0; };  // mask_fusion_conv, unet.py:298-305
enum TapeKind { TAPE_RES, TAPE_LIN, TAPE_MID, TAPE_CONV, TAPE_INJ };          // which of Plan's record vectors `idx` points into
struct TapeItem { TapeKind kind; int idx; };   // in forward order

struct Plan {                 // one launch plan + activation arena for up to maxB rows
    int maxB = 0, H = 0, W = 0;
    std::vector<Op> ops;
    std::vector<std::string> op_kernel, op_what;  // parallel to ops: kernel family, reference module it serves
    std::vector<double> op_flops;                  // algorithmic FLOPs per sample of that launch
    std::vector<char> op_param_only;               // backward plans: the launch's only products are parameter gradients (fc_unet_vjp_x leaves it out)
    std::vector<double> op_bytes_ps, op_bytes_fixed;   // algorithmic HBM bytes of that launch: per sample (activations in + out, each once) and per launch (weights); 0 = not stated
    std::vector<void*> allocs;
    double flops = 0.0;            // per sample, the reference's arithmetic (2 x MACs of every module as upstream computes it)
    double flops_executed = 0.0;   // per sample, what the launches execute (less where upsampling is folded into the weights)
    float *t_emb = nullptr, *ss = nullptr;
    std::map<std::string, Act> named;              // debug taps: block outputs by reference module name
    std::vector<ResRec> res; std::vector<LinRec> lin; std::vector<MidRec> mid; std::vector<ConvRec> convs; std::vector<InjRec> inj;
    FuseRec fuse;
    std::vector<TapeItem> tape;
    Act x0, head;                                   // init_conv output, final_res_block output
    int n_meet = 0;                                 // launches whose workgroups wait for each other (fused Block tails across workgroups)
    std::vector<unsigned*> fin_sync;                // their arrival counters (fc_debug_unet_break_meeting)
    std::vector<int> fin_kind;                      // ... and what waits on them: 0 a convolution's Block tail, 1 the linear attention's close
    // the step-closing flavour of final_res_block's closing launch (conv_dev.h FL_STEP): its device block, or null when the plan's launch
    // is not the one that flavour is compiled for; the launch's arrival counters and workgroups per sample (the block's base epochs)
    StepClose* step_blk = nullptr;
    const unsigned* step_sync = nullptr;
    int step_gsz = 0;
    void release() {
        for (void* p : allocs) dev_free(p);
        *this = Plan();
    }
};

struct PackOp { int64_t src, dst; PackJob job; };   // a job whose pointers are still offsets into `raw` / `packed` (until alloc_device)

static const char* const kTileNames[] = {"conv_igemm<M128,N32>", "conv_igemm<M128,N64>", "conv_igemm<M64,N32,K2>", "conv_igemm<M32,N32,K4>",
                                         "conv_igemm<M64,N64,K2>", "conv_igemm<M256,N64>"};

// Parameters as the reference stores them (`raw`, flat, table order, every tensor 16-byte aligned) plus the operand
// layouts the kernels read (`packed`), and the list of re-layout launches that turns one into the other.
struct ParamStore {
    std::vector<Param> params;
    std::unordered_map<std::string, int> pidx;
    int64_t raw_numel = 0, packed_numel = 0;
    float *raw = nullptr, *packed = nullptr;
    std::unordered_map<std::string, int64_t> pk;  // name -> offset into packed
    std::vector<PackOp> packops;
    PackTable pack_table;                          // all of `packops` as one launch
    bool loaded = false;

    bool want_b3 = false;   // also keep 3x3 / 1x1 conv weights as split bf16 (PACK_CONV_B3): the codecs, for their opt-in split-bf16 arithmetic
    std::unordered_map<int64_t, int64_t> b3_of;   // packed offset of a weight -> packed offset of its split-bf16 copy
    const float* B3(const float* w) const {         // the split-bf16 copy of packed weight pointer `w`, or null
        auto it = b3_of.find(w - packed);
        return it == b3_of.end() ? nullptr : packed + it->second;
    }
    bool want_k8 = false;   // also keep 3x3 / 1x1 conv weights in the k-step-quad layout (PACK_CONV_K8) where the shapes allow: the U-Net's low-resolution layers
    // the k-step-quad copy of a convolution weight, or null when there is none
    const float* P8(const std::string& n) const { auto it = pk.find(n + "#k8"); return it == pk.end() ? nullptr : packed + it->second; }
    const float* R(const std::string& n) const { return raw + params[pidx.at(n)].offset; }
    const float* P(const std::string& n) const { return packed + pk.at(n); }
    bool has(const std::string& n) const { return pidx.count(n) != 0; }
    // the bias of layer `n` as its convolution reads it: the packed copy where one was declared (decl_conv_pad's zero-padded slot), else
    // the raw tensor, or null for a layer declared without a bias (to_qkv, NATTEN's qkv / proj)
    const float* bias(const std::string& n) const {
        auto it = pk.find(n + ".bias");
        if (it != pk.end()) return packed + it->second;
        return has(n + ".bias") ? R(n + ".bias") : nullptr;
    }

    void declare(const std::string& name, std::initializer_list<int64_t> shape) {
        Param p;
        p.name = name;
        p.numel = 1;
        int i = 0;
        for (int64_t s : shape) { p.shape[i++] = s; p.numel *= s; }
        p.offset = raw_numel;
        raw_numel += (p.numel + 3) & ~3ll;  // keep every tensor 16-byte aligned inside `raw`
        pidx[name] = (int)params.size();
        params.push_back(p);
    }
    int64_t pk_alloc(const std::string& name, int64_t numel) {
        const int64_t off = packed_numel;
        pk[name] = off;
        packed_numel += (numel + 3) & ~3ll;
        return off;
    }
    int64_t off(const std::string& n) const { return params[pidx.at(n)].offset; }
    // parameter `n` goes, laid out as `job` says, to offset `dst` of `packed`
    void pack(const std::string& n, int64_t dst, const PackJob& job) { packops.push_back(PackOp{off(n), dst, job}); }
    void decl_conv(const std::string& n, int O, int I, int K, bool bias = true) {
        declare(n + ".weight", {O, I, K, K});
        if (bias) declare(n + ".bias", {O});
        const int64_t dst = pk_alloc(n + ".weight", (int64_t)O * I * K * K);
        pack(n + ".weight", dst, pack_job_conv(O, I, K * K));
        if (want_b3 && (K == 3 || K == 1)) {
            const int Ipad = (I + 15) / 16 * 16;
            const int64_t d3 = pk_alloc(n + ".weight#b3", (int64_t)O * Ipad * K * K);
            pack(n + ".weight", d3, pack_job_conv_b3(O, I, K * K, Ipad));
            b3_of[dst] = d3;
        }
        if (want_k8 && (K == 3 || K == 1) && I % 32 == 0 && O % 32 == 0)
            pack(n + ".weight", pk_alloc(n + ".weight#k8", (int64_t)O * I * K * K), pack_job_conv_k8(O, I, K * K));
    }
    // Conv2d whose channel counts need not be multiples of 4 (the pixel-space ends of the codecs): operands zero-padded to Opad / Ipad;
    // `packed_bias`: the bias too, copied into a zero-initialised packed slot of Opad floats (P(n + ".bias"))
    void decl_conv_pad(const std::string& n, int O, int I, int K, int Opad, int Ipad, bool packed_bias) {
        declare(n + ".weight", {O, I, K, K});
        declare(n + ".bias", {O});
        pack(n + ".weight", pk_alloc(n + ".weight", (int64_t)Opad * Ipad * K * K), pack_job_conv_pad(O, I, K * K, Opad, Ipad));
        if (packed_bias) pack(n + ".bias", pk_alloc(n + ".bias", Opad), pack_job_copy(O));
    }
    // Downsample's 1x1 convolution over the space-to-depth rearrangement, [O][4C][1][1], as a 2x2 stride-2 convolution (PACK_S2D)
    void decl_conv_s2d(const std::string& n, int O, int C) {
        declare(n + ".weight", {O, 4 * C, 1, 1});
        declare(n + ".bias", {O});
        pack(n + ".weight", pk_alloc(n + ".weight", (int64_t)O * 4 * C), pack_job_s2d(O, C));
    }
    // a 3x3 convolution behind nn.Upsample(nearest, x2): besides the plain packed copy, the four parity kernels of the folded form (PACK_UP4 / PACK_UP4_B3)
    void decl_conv_up2(const std::string& n, int O, int I) {
        decl_conv(n, O, I, 3);
        const int64_t d4 = pk_alloc(n + ".weight#up4", (int64_t)16 * O * I);
        pack(n + ".weight", d4, pack_job_up4(O, I));
        if (want_b3) {
            const int Ipad = (I + 15) / 16 * 16;
            const int64_t d3 = pk_alloc(n + ".weight#up4b3", (int64_t)16 * O * Ipad);
            pack(n + ".weight", d3, pack_job_up4_b3(O, I, Ipad));
            for (int par = 0; par < 4; ++par) b3_of[d4 + (int64_t)par * 4 * O * I] = d3 + (int64_t)par * 4 * O * Ipad;
        }
    }
    const float* PUP(const std::string& n) const {     // [parity][4 taps][I][O], or null when the layer was not declared with decl_conv_up2
        auto it = pk.find(n + "#up4");
        return it == pk.end() ? nullptr : packed + it->second;
    }
    void decl_linear_t(const std::string& n, int O, int I, bool bias = true) {  // stored transposed [I][O]
        declare(n + ".weight", {O, I});
        if (bias) declare(n + ".bias", {O});
        pack(n + ".weight", pk_alloc(n + ".weight", (int64_t)O * I), pack_job_transpose(O, I, O, 0));
    }
    // parameter `n` into a slice of the named packed buffer `buf`: a Linear [R][Cc] transposed into columns col0 .. col0 + R of its rows of
    // ld floats; a vector of R floats copied to elements col0 .. col0 + R
    void pack_transpose_into(const std::string& buf, const std::string& n, int R, int Cc, int ld, int col0) { pack(n, pk.at(buf), pack_job_transpose(R, Cc, ld, col0)); }
    void pack_copy_into(const std::string& buf, const std::string& n, int R, int col0) { pack(n, pk.at(buf) + col0, pack_job_copy(R)); }
    void decl_norm(const std::string& n, int C) {
        declare(n + ".weight", {C});
        declare(n + ".bias", {C});
    }
    int alloc_device() {
        FC_TRY(dev_alloc(reinterpret_cast<void**>(&raw), (size_t)(raw_numel ? raw_numel : 4) * sizeof(float), "params.raw"));
        FC_TRY(dev_alloc(reinterpret_cast<void**>(&packed), (size_t)(packed_numel ? packed_numel : 4) * sizeof(float), "params.packed"));
        FC_HIP(hipMemset(raw, 0, (size_t)(raw_numel ? raw_numel : 4) * sizeof(float)));
        std::vector<PackJob> jobs;
        for (const PackOp& o : packops) jobs.push_back(o.job.at(raw + o.src, packed + o.dst));
        return pack_table_build(jobs, &pack_table);
    }
    void free_device() {
        pack_table.release();
        if (raw) dev_free(raw);
        if (packed) dev_free(packed);
        raw = packed = nullptr;
    }
    int run_pack(hipStream_t s) const { return pack_table_launch(pack_table, s); }
    // flat fp32 vector in table order (padded layout) -> raw -> packed
    int load(const float* flat, int64_t numel, int on_device, hipStream_t s) {
        if (numel != raw_numel) return fail(FC_E_ARG, "load_params: expected " + std::to_string(raw_numel) + " floats (padded table layout)");
        FC_HIP(hipMemcpyAsync(raw, flat, (size_t)numel * sizeof(float), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        FC_TRY(run_pack(s));
        if (!on_device) FC_HIP(hipStreamSynchronize(s));  // the host buffer may be freed by the caller on return
        loaded = true;
        return FC_OK;
    }
    int info(int i, const char** name, int64_t shape[4], int64_t* offset) const {
        if (i < 0 || i >= (int)params.size()) return fail(FC_E_ARG, "param_info: index out of range");
        const Param& p = params[i];
        if (name) *name = p.name.c_str();
        if (shape) for (int k = 0; k < 4; ++k) shape[k] = p.shape[k];
        if (offset) *offset = p.offset;
        return FC_OK;
    }
};

struct PlanBuilder {
    Plan* pl = nullptr;
    int B = 0;  // max batch
    int err = FC_OK;
    std::string scope;  // reference module the ops being emitted belong to
    int* fin_err_word = nullptr;   // device word a timed-out fused tail sets (owned by the handle the plan belongs to)
    int conv_prec = 0;             // ConvArgs::prec of every convolution this builder emits (codec plans: 1 = split-bf16 on request)
    const ParamStore* store = nullptr;   // the model: where layer() finds a layer's operands and bind_out() the split-bf16 copy of a weight
    Act step_out;                  // set around the Block whose closing launch may close the sampler's step too: the tensor that flavour writes (conv_fin)

    // guard: 0 always | 1 only when the call has a mask | 2 only when it runs mask_fusion_conv | 3 only when it has NO mask | 4 mask but no fusion
    int guard = 0;
    // backward plans: the entries pushed while this is set produce nothing the data-gradient chain towards d(x) reads (Plan::op_param_only)
    bool param_only = false;
    // flops: what the launch executes per sample (per-launch tables, rooflines); flops_ref (> 0): what the reference's arithmetic for the same
    // module is, when that differs (folded upsampling) -- Plan::flops, the per-sample figure of SURVEY 8(d), adds up the reference's
    void push(Op op, const std::string& kernel, double flops = 0.0, double bytes_ps = 0.0, double bytes_fixed = 0.0, double flops_ref = 0.0) {
        if (guard) {
            const int g = guard;
            Op inner = std::move(op);
            op = [inner, g](const FwdCtx& c, hipStream_t s) -> int {
                const bool on = g == 1 ? c.mask != nullptr : g == 2 ? c.mask_fuse != 0 : g == 3 ? c.mask == nullptr : (c.mask != nullptr && !c.mask_fuse);
                return on ? inner(c, s) : FC_OK;
            };
        }
        pl->ops.push_back(std::move(op));
        pl->op_kernel.push_back(kernel);
        pl->op_what.push_back(scope);
        pl->op_flops.push_back(flops);
        pl->op_param_only.push_back(param_only ? 1 : 0);
        pl->op_bytes_ps.push_back(bytes_ps);
        pl->op_bytes_fixed.push_back(bytes_fixed);
        pl->flops += flops_ref > 0.0 ? flops_ref : flops;
        pl->flops_executed += flops;
    }
    float* dmalloc(size_t floats) {
        void* p = nullptr;
        if (dev_alloc(&p, (floats ? floats : 1) * sizeof(float), scope.c_str()) != FC_OK) { err = fail(FC_E_HIP, "hipMalloc failed while reserving the arena"); return nullptr; }
        pl->allocs.push_back(p);
        return static_cast<float*>(p);
    }
    // a host table copied into a buffer of the arena (before returning: the vector may die); null with `err` set on failure
    template <class T> T* upload(const std::vector<T>& v) {
        T* d = reinterpret_cast<T*>(dmalloc((v.size() * sizeof(T) + 3) / 4 + 4));
        if (d && hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) {
            err = fail(FC_E_HIP, "hipMemcpy failed while uploading a plan table");
            return nullptr;
        }
        return d;
    }
    std::multimap<size_t, float*> pool;   // buffers handed back by release(): later tensors of the same size reuse them
    Act act(int C, int H, int W) {
        Act a; a.C = C; a.H = H; a.W = W;
        const size_t n = (size_t)B * H * W * C;
        auto it = pool.find(n);
        if (it != pool.end()) { a.p = it->second; pool.erase(it); }
        else a.p = dmalloc(n);
        return a;
    }
    // The plan is a fixed sequence on one stream, so a buffer whose last reader has been emitted can serve a later tensor.
    // keep_all (debug taps, tests only): nothing goes back to the pool, so every tensor keeps its own memory after a run and tap()
    // records it in Plan::named.
    bool keep_all = false;
    void release(const Act& a) { if (a.p && !keep_all) pool.emplace((size_t)B * a.H * a.W * a.C, a.p); }
    void tap(const std::string& name, const Act& a) { if (keep_all && !err) pl->named[name] = a; }
    Stat stat(int G, int T, float n_t) { Stat s; s.G = G; s.T = T; s.n_t = n_t; s.p = dmalloc((size_t)B * G * T * 2); return s; }

    static SrcXform xf_of(const Stat& st, int mode, const float* gamma, const float* beta, const float* ss = nullptr, int ss_stride = 0,
                          float eps = 1e-5f) {
        SrcXform x;
        x.mode = mode; x.stats = st.p; x.G = st.G; x.T = st.T; x.n_t = st.n_t;
        x.gamma = gamma; x.beta = beta; x.ss = ss; x.ss_stride = ss_stride; x.eps = eps;
        return x;
    }

    // Algorithmic HBM bytes of one convolution launch: every input / output / residual element once per sample, the
    // weights once per launch -- what a kernel with perfect on-chip reuse would move.
    static double conv_bytes_ps(const ConvArgs& a) {
        double e = (double)a.Hs * a.Ws * a.Cin + (double)a.H * a.W * a.Cout;
        if (a.res_out) e += (double)a.H * a.W * a.Cout;
        if (a.add) e += (double)a.H * a.W * a.Cout;
        if (a.fin.res) e += (double)a.H * a.W * a.Cout;
        if (a.w_batch_stride) e += (double)a.KS * a.KS * a.Cin * a.Cout;
        return 4.0 * e;
    }
    static double conv_bytes_fixed(const ConvArgs& a) {
        double e = a.w_batch_stride ? 0.0 : (double)a.KS * a.KS * a.Cin * a.Cout;
        if (a.res_w) e += (double)a.Cin * a.Cout;
        return 4.0 * e;
    }

    // ---- The vocabulary of a launch site.  A site states only what is special about its layer: it takes the ordinary arguments from one of
    // these and sets on the result the fields that differ (stride, ups, out_act, add, stats_post, s1, s0.xf, w_batch_stride, w4, res_*, ...).

    // a tensor as a convolution source, read through `xf`
    static ConvSrc src(const Act& x, const SrcXform& xf = SrcXform()) { ConvSrc s; s.p = x.p; s.C = x.C; s.xf = xf; return s; }
    // the "same" stride-1 KS x KS convolution of x with weights w (packed) and `bias` (or null)
    static ConvArgs conv_on(const Act& x, int KS, const float* w, const float* bias) {
        ConvArgs a;
        a.s0 = src(x); a.Hs = x.H; a.Ws = x.W; a.KS = KS; a.pad = KS / 2; a.w = w; a.bias = bias;
        return a;
    }
    // ... of the layer `name` of the model in `store`.  The k-step-quad operands (w4 / res_w4) stay with the sites that want them:
    // attaching a layer's `#k8` copy changes the route its launch takes.
    ConvArgs layer(const std::string& name, const Act& x, int KS) const { return conv_on(x, KS, store->P(name + ".weight"), store->bias(name)); }
    // What follows from the output tensor and the builder.  Precision and the split-bf16 copy are set for every launch alike: the paths
    // that left them out before (conv_fin, the U-Net's stem and injections) belong to the U-Net's builders, whose conv_prec is 0.
    void bind_out(ConvArgs& a, const Act& out) const {
        a.B = B; a.H = out.H; a.W = out.W; a.Cout = out.C; a.out = out.p;
        a.Cin = a.s0.C + a.s1.C;
        a.prec = conv_prec;
        if (conv_prec && store && !a.w_batch_stride) a.w_b3 = store->B3(a.w);
    }
    // y = act(gn(h)) as finalize's arguments; a site adds res / xf_res / act_after_add / stats_out
    static FinalizeArgs fin_of(const Act& h, const SrcXform& xf, const Act& y) {
        FinalizeArgs f;
        f.h = h.p; f.xf = xf; f.y = y.p; f.HW = h.H * h.W; f.C = h.C;
        return f;
    }
    void finalize(const FinalizeArgs& f) {
        if (!err) push([f](const FwdCtx& c, hipStream_t s) { FinalizeArgs g = f; g.B = c.B; return finalize_launch(g, s); }, "finalize");
    }
    // a new tensor holding act(gn(h)), for the consumers that read it raw
    Act activated(const Act& h, const SrcXform& xf) {
        if (err) return Act();      // a builder in error allocates nothing more
        Act y = act(h.C, h.H, h.W);
        finalize(fin_of(h, xf, y));
        return y;
    }
    // GroupNorm(G) statistics of a stored tensor in a launch of their own
    Stat gn_stats(const Act& a, int G) {
        Stat st = stat(G, 1, (float)(a.H * a.W * (a.C / G)));
        float* sp = st.p; const float* xp = a.p; const int HW = a.H * a.W, C = a.C;
        push([=](const FwdCtx& c, hipStream_t s) { return gn_stats_launch(xp, sp, c.B, HW, C, G, s); }, "gn_stats");
        return st;
    }

    // Emits one implicit-GEMM launch (plus a standalone statistics pass when the output has < 16 pixels per sample).
    // `want_G` > 0 asks for GroupNorm partials of the output; returns them in *st.
    void conv(ConvArgs a, const Act& out, int want_G, Stat* st) {
        if (err) return;
        bind_out(a, out);
        const bool fused = want_G > 0 && (out.H * out.W) % 16 == 0;
        ConvGeom g;
        if (fused) { a.Gout = want_G; a.stats_out = reinterpret_cast<float*>(1); }  // placeholder: geometry only
        if ((err = conv_plan(a, TILE_AUTO, &g)) != FC_OK) return;
        if (fused) { *st = stat(want_G, g.T, g.n_t); a.stats_out = st->p; }
        const int tile = g.tile;
        double fl = 2.0 * out.H * out.W * a.KS * a.KS * (double)a.Cin * a.Cout;
        if (a.res_out) fl += 2.0 * out.H * out.W * (double)a.Cin * a.Cout;
        push([a, tile](const FwdCtx& c, hipStream_t s) { ConvArgs b = a; b.B = c.B; return conv_launch(b, tile, s); }, kTileNames[tile], fl,
             conv_bytes_ps(a), conv_bytes_fixed(a));
        if (fused) fold_partials(st);
        if (want_G > 0 && !fused) *st = gn_stats(out, want_G);
    }

private:
    // many tiles per sample (large images): fold the partials once instead of in every consumer workgroup
    void fold_partials(Stat* st) {
        if (st->T <= 16) return;
        const Stat raw = *st;
        *st = stat(raw.G, 1, raw.n_t * (float)raw.T);
        const float* ip = raw.p; float* op = st->p;
        const int G = raw.G, T = raw.T; const float nt = raw.n_t;
        push([=](const FwdCtx& c, hipStream_t s) { return gn_fold_launch(ip, op, c.B, G, T, nt, s); }, "gn_fold");
    }

public:
    // nn.Upsample(nearest, x2) + 3x3 convolution as four 2x2 convolutions on the low-resolution input, one per output parity, with the taps
    // that fall on the same source pixel summed at pack time (ParamStore::decl_conv_up2): 16 instead of 36 multiply-adds per 2x2 output
    // block and channel pair -- exact in real arithmetic, a different summation order in fp32.  One launch carries the four classes
    // (ConvArgs::par4).  `w4` = PUP(name); x low resolution, out 2x.  Returns false, emitting nothing, when the shape is not covered
    // (the caller then emits the 3x3 convolution over the upsampled window).
    bool conv_up2(const Act& x, const float* w4, const float* bias, const Act& out, int want_G, Stat* st) {
        if (err || !w4) return false;
        static const bool no_fold = [] { const char* e = std::getenv("FLOCODER_AMD_UPS_FOLD"); return e && std::string(e) == "0"; }();
        if (no_fold || (want_G > 0 && (x.H * x.W) % 16 != 0)) return false;
        ConvArgs a = conv_on(x, 2, w4, bias);
        a.pad = 0;
        bind_out(a, out);
        a.H = x.H; a.W = x.W;      // the launch's grid is the low-resolution one: each of its pixels writes a 2x2 block of `out` (out_sh)
        a.par4 = 1; a.out_sh = 1; a.stats_tmul = 4; a.pad_y = 1; a.pad_x = 1;
        const bool fused = want_G > 0;
        ConvGeom g;
        if (fused) { a.Gout = want_G; a.stats_out = reinterpret_cast<float*>(1); }
        if (conv_plan(a, TILE_AUTO, &g) != FC_OK || !g.pipe) return false;
        if (fused) { *st = stat(want_G, 4 * g.T, g.n_t); a.stats_out = st->p; }
        const int tile = g.tile;
        const double fl = 2.0 * out.H * out.W * 4.0 * (double)a.Cin * a.Cout;      // four taps per OUTPUT pixel
        push([a, tile](const FwdCtx& c, hipStream_t s) { ConvArgs b = a; b.B = c.B; return conv_launch(b, tile, s); }, kTileNames[tile], fl,
             4.0 * ((double)x.H * x.W * a.Cin + (double)out.H * out.W * a.Cout), 4.0 * 16.0 * a.Cin * a.Cout,
             2.0 * out.H * out.W * 9.0 * (double)a.Cin * a.Cout);
        if (fused) fold_partials(st);
        return true;
    }

    // A convolution whose epilogue finishes the Block: out = SiLU(GroupNorm(conv)) + res, the GroupNorm statistics exchanged between
    // the workgroups of a sample through a counter (ConvFin).  Returns false, emitting nothing, when the launch cannot keep its whole
    // grid resident or the shape is outside the fused tail's conditions -- the caller then emits conv + finalize.
    bool conv_fin(ConvArgs a, const Act& out, int G, const float* gamma, const float* beta, const float* res, bool want_gn1, Stat* gn1,
                  bool only_local = false) {
        if (err) return false;
        bind_out(a, out);
        if ((out.H * out.W) % 16) return false;
        a.Gout = G; a.stats_out = reinterpret_cast<float*>(16);
        a.fin.gamma = gamma; a.fin.beta = beta; a.fin.res = res;
        if (want_gn1) a.fin.gn1_out = reinterpret_cast<float*>(16);   // placeholder: the geometry (and the occupancy query behind the
                                                                      // residency check) must see the flavour the launch will use
        ConvGeom g;
        if (conv_plan(a, TILE_AUTO, &g) != FC_OK || !g.pipe) return false;
        if (only_local && !g.fin_local) return false;    // the cross-workgroup meeting costs what the finalize launch costs; the local form is free
        Stat st = stat(G, g.T, g.n_t);
        a.stats_out = st.p;
        if (want_gn1) { *gn1 = stat(1, g.T1, g.n_t1); a.fin.gn1_out = gn1->p; }
        unsigned* sync = reinterpret_cast<unsigned*>(dmalloc((size_t)g.groups + 1));
        if (err) return false;
        if (hipMemset(sync, 0, ((size_t)g.groups + 1) * sizeof(unsigned)) != hipSuccess) { err = fail(FC_E_HIP, "hipMemset failed"); return false; }
        const size_t ngran = (size_t)B * G * g.T * 2;                       // one 8-byte {epoch, value} granule per partial statistic
        a.fin.gran = reinterpret_cast<unsigned long long*>(dmalloc(2 * ngran));
        if (err) return false;
        if (hipMemset(a.fin.gran, 0, ngran * sizeof(unsigned long long)) != hipSuccess) { err = fail(FC_E_HIP, "hipMemset failed"); return false; }   // tag 0 = never a live epoch
        a.fin.sync = sync;
        a.fin.err = fin_err_word ? fin_err_word : reinterpret_cast<int*>(sync + g.groups);   // the handle's error word (one per object)
        if (!g.fin_local) { ++pl->n_meet; pl->fin_sync.push_back(sync); pl->fin_kind.push_back(0); }
        const int tile = g.tile;
        // the launch that may close the sampler's step as well (`step_out`): only when it is exactly the one that flavour is compiled for
        float* sout = nullptr;
        if (step_out.p && step_out.C == out.C && step_out.H == out.H && step_out.W == out.W && conv_step_close_possible(a, tile)) {
            pl->step_blk = reinterpret_cast<StepClose*>(dmalloc(sizeof(StepClose) / sizeof(float) + (size_t)B));
            if (err) return false;
            pl->step_sync = sync; pl->step_gsz = g.gsz;
            sout = step_out.p;
        }
        const double fl = 2.0 * out.H * out.W * a.KS * a.KS * (double)a.Cin * a.Cout;
        push([a, tile, sout](const FwdCtx& c, hipStream_t s) {
            ConvArgs b = a; b.B = c.B;
            if (c.step && sout) { b.fin.step = c.step; b.out = sout; }
            return conv_launch(b, tile, s);
        }, std::string(kTileNames[tile]) + "+fin", fl, conv_bytes_ps(a), conv_bytes_fixed(a));
        return true;
    }

    // Single-head softmax attention over the h*w tokens of x with d = C (diffusers' VAE mid-block attention, VQGAN's AttnBlock):
    //   out = proj(softmax(q k^T / sqrt(C)) v) + x,   q/k/v = 1x1 conv of GroupNorm(x)
    // as three 1x1 convs with the norm in their loader, a batched transpose, two per-sample-weight GEMMs on the conv kernel and a
    // one-pass row softmax.  `names`: the model's q, k, v and output projections (1x1 convolutions or transposed Linears, packed [Cin][Cout]);
    // want_G > 0 also returns GroupNorm partials of the sum.
    struct AttnNames { std::string q, k, v, out; };
    Act attention_block(const Act& x, const SrcXform& norm_x, const AttnNames& names, int want_G, Stat* so) {
        const int C = x.C, hw = x.H * x.W;
        Act q = act(C, x.H, x.W), k = act(C, x.H, x.W), vv = act(C, x.H, x.W);
        const std::string* proj[3] = {&names.q, &names.k, &names.v};
        const Act* outs[3] = {&q, &k, &vv};
        for (int i = 0; i < 3; ++i) {
            ConvArgs a = layer(*proj[i], x, 1);
            a.s0.xf = norm_x;
            conv(a, *outs[i], 0, nullptr);
        }
        float* kt = dmalloc((size_t)B * C * hw);                    // k^T per sample: [C][n]
        const float* kp = k.p;
        push([=](const FwdCtx& c, hipStream_t s) { return transpose_batched_launch(kp, kt, c.B, hw, C, s); }, "transpose");
        Act sc = act(hw, x.H, x.W);                                 // scores [B][n][n]
        {
            ConvArgs a = conv_on(q, 1, kt, nullptr);
            a.w_batch_stride = C * hw;
            conv(a, sc, 0, nullptr);
        }
        float* sp = sc.p;
        const float scale = 1.0f / sqrtf((float)C);
        push([=](const FwdCtx& c, hipStream_t s) { return softmax_rows_launch(sp, (long)c.B * hw, hw, scale, s); }, "softmax_rows");
        Act o = act(C, x.H, x.W);
        {
            ConvArgs a = conv_on(sc, 1, vv.p, nullptr);
            a.w_batch_stride = hw * C;
            conv(a, o, 0, nullptr);
        }
        Act out = act(C, x.H, x.W);
        {
            ConvArgs a = layer(names.out, o, 1);
            a.add = x.p; a.stats_post = 1;
            conv(a, out, want_G, so);
        }
        tap(scope + ".q", q); tap(scope + ".k", k); tap(scope + ".v", vv); tap(scope + ".p", sc); tap(scope + ".o", o);   // .p: after the softmax
        release(q); release(k); release(vv); release(sc); release(o);
        return out;
    }
};

inline int run_plan(const Plan& pl, const FwdCtx& c, hipStream_t s) {
    for (const Op& op : pl.ops) FC_TRY(op(c, s));
    return FC_OK;
}

// Measurement: every launch of `pl` timed alone -- `repeats` back-to-back launches between two HIP events on `s` (ops only read their
// inputs, so repeating one is idempotent; host launch gaps do not pollute kernels that run longer than a launch takes to issue).
// ms_out[i] = average milliseconds of op i.  `after_op` (optional) runs behind op i's closing event, outside its timing.  Synchronises.
inline int profile_plan(const Plan& pl, const FwdCtx& c, int repeats, float* ms_out, int n_out, hipStream_t s,
                        const std::function<int(int)>& after_op = nullptr) {
    const int n = (int)pl.ops.size();
    if (n_out < n) return fail(FC_E_ARG, "profile_ops: output array too small");
    FC_TRY(run_plan(pl, c, s));   // warm: every buffer holds finite data
    std::vector<hipEvent_t> ev(2 * n);
    for (auto& e : ev) FC_HIP(hipEventCreate(&e));
    int rc = FC_OK;
    for (int i = 0; i < n && rc == FC_OK; ++i) {
        (void)hipEventRecord(ev[2 * i], s);
        for (int r = 0; r < repeats && rc == FC_OK; ++r) rc = pl.ops[i](c, s);
        (void)hipEventRecord(ev[2 * i + 1], s);
        if (after_op && rc == FC_OK) rc = after_op(i);
    }
    (void)hipStreamSynchronize(s);
    for (int i = 0; i < n; ++i) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]);
        ms_out[i] = ms / repeats;
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    return rc;
}

}  // namespace fc
