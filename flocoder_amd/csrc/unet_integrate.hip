// The integrators of the velocity U-Net: fixed-grid Euler / RK4 (fc_unet_integrate), likelihood / inversion (fc_unet_log_likelihood) and
// measurement guidance (fc_unet_integrate_guided) on the RK4 grid, the stochastic sampler (fc_unet_integrate_sde) and adaptive RK45
// (fc_unet_integrate_rk45*).  Host code only: the kernels are ode.hip's, the forward is the handle's launch plan (unet.hip).  Every call
// runs on the library's own stream inside one CallFrame; its state is fc_unet::ig.  Every RK4 integrator enqueues its intervals through
// enqueue_rk4_interval, the one place that holds rk4_step's launch sequence and stage constants.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>

#include "plan.h"
#include "unet_priv.h"

using namespace fc;

namespace fc {

// ------------------------------------------------------------------------------------------- state
void IntegratorState::drop_graphs() {
    for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
    graphs.clear();
}
void IntegratorState::release_plan() {
    drop_graphs();
    for (void* p : allocs) dev_free(p);
    static_cast<IntegratorPlanState&>(*this) = IntegratorPlanState{};
}
void IntegratorState::release_handle() {
    release_plan();
    for (void* p : {(void*)ts_dev, (void*)rk_ev, (void*)pre}) if (p) dev_free(p);
    if (stream) (void)hipStreamDestroy(stream);
    if (ev_in) (void)hipEventDestroy(ev_in);
    if (ev_out) (void)hipEventDestroy(ev_out);
    if (rk_host) (void)hipHostFree(rk_host);
    if (ev_rk) (void)hipEventDestroy(ev_rk);
}

// integrator state for `rows` U-Net rows
int alloc_integrator(fc_unet* u, int rows, int H, int W) {
    IntegratorState& ig = u->ig;
    const size_t nstate = (size_t)rows * u->cfg.channels * H * W;
    for (float** b : {&ig.y, &ig.xs, &ig.k1, &ig.k2, &ig.k3, &ig.v2, &ig.mask_own}) FC_TRY(ig.get(b, nstate, "integrator"));
    FC_TRY(ig.get(&ig.tvec, rows, "integrator"));
    FC_TRY(ig.get(&ig.sc, 4, "integrator"));
    FC_TRY(ig.get(&ig.step, 4, "integrator"));
    return ig.get(&ig.ids_own, rows, "integrator");
}

// ------------------------------------------------------------------------------------------- call frame
// One integrator call.  begin() derives what every path derives from its arguments and checks that the handle can run them; nothing is
// touched yet.  enter() moves the call onto the library stream: the hand-over from the caller's stream, the call's class ids and mask
// copied into the library's own buffers, the meeting guard.  leave() hands back; a call that returns early after enter() leaves through
// the destructor, so the caller's stream is ordered behind whatever the library stream still holds and the meeting guard knows this
// handle's last plan -- whichever FC_TRY failed.  A fixed-grid entry point reads: checks, begin, own allocations, enter, prologue, own
// staging, intervals, finish.
struct CallFrame {
    fc_unet* u = nullptr;
    hipStream_t caller = nullptr, s = nullptr;
    const int64_t* ids = nullptr;
    const float* mask = nullptr;
    bool has_ids = false, cfg_on = false, entered = false;
    int B = 0, rows = 0, mask_mode = 0, n = 0;      // rows: U-Net rows per evaluation (2B with CFG); n: unknowns of the batch
    size_t nbytes = 0;                              // of the state (and of the mask)

    int begin(fc_unet* u_, int B_, int H, int W, const int64_t* ids_, float cfg_strength, const float* mask_, int mask_is_ones, void* stream) {
        u = u_; B = B_; ids = ids_; mask = mask_; caller = static_cast<hipStream_t>(stream); s = u->ig.stream;
        has_ids = ids != nullptr && u->cfg.n_classes > 0;
        cfg_on = has_ids && cfg_strength != 0.0f;   // sampling.py:69
        rows = cfg_on ? 2 * B : B;
        mask_mode = (mask && u->cfg.mask_cond) ? (mask_is_ones ? 2 : 1) : 0;
        n = B * u->cfg.channels * H * W; nbytes = (size_t)n * sizeof(float);
        FC_TRY(check_ready(u, rows, H, W));
        FC_TRY(check_poison(u));
        FC_HIP(hipSetDevice(u->device));
        return FC_OK;
    }
    int enter() {
        u->arena_touched(0);
        // the library stream picks up after everything already queued on the caller's stream
        FC_HIP(hipEventRecord(u->ig.ev_in, caller));
        FC_HIP(hipStreamWaitEvent(s, u->ig.ev_in, 0));
        entered = true;
        if (has_ids) FC_HIP(hipMemcpyAsync(u->ig.ids_own, ids, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
        if (mask_mode) FC_HIP(hipMemcpyAsync(u->ig.mask_own, mask, nbytes, hipMemcpyDeviceToDevice, s));
        return meet_enter(u, s);
    }
    int leave() {
        entered = false;
        FC_TRY(meet_leave(u, s));
        FC_HIP(hipEventRecord(u->ig.ev_out, s));
        FC_HIP(hipStreamWaitEvent(caller, u->ig.ev_out, 0));
        return FC_OK;
    }
    // the tail of every fixed-grid call: the state back into the caller's tensor, then leave()
    int finish(float* x_dev) {
        FC_HIP(hipMemcpyAsync(x_dev, u->ig.y, nbytes, hipMemcpyDeviceToDevice, s));
        return leave();
    }
    ~CallFrame() {
        if (!entered) return;
        const std::string first = fc_last_error();   // the error that ended the call stays the one reported
        if (leave() != FC_OK) set_error(first);
    }
};

}  // namespace fc

extern "C" {

// ------------------------------------------------------------------------------------------- graph cache
static uint32_t fbits(float f) { uint32_t v; std::memcpy(&v, &f, 4); return v; }

// the kernels read and write these as float4 (NULL passes); `msg`: the entry point's own text
static int check_aligned16(std::initializer_list<const void*> ptrs, const char* msg) {
    for (const void* p : ptrs) if (reinterpret_cast<uintptr_t>(p) & 15) return fail(FC_E_ARG, msg);
    return FC_OK;
}

// FLOCODER_AMD_NO_GRAPH: every integrator enqueues its launches directly instead of capturing and replaying graphs
static bool no_graph() {
    static const bool v = std::getenv("FLOCODER_AMD_NO_GRAPH") != nullptr;
    return v;
}

// the graph cached under `key`; on first use it is captured from `enqueue` on `s` and instantiated
static int cached_graph(fc_unet* u, const GraphKey& key, hipStream_t s, const std::function<int()>& enqueue, hipGraphExec_t* out) {
    IntegratorState& ig = u->ig;
    auto it = ig.graphs.find(key);
    if (it == ig.graphs.end()) {
        hipGraph_t graph = nullptr;
        FC_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        const int r = enqueue();
        const hipError_t e = hipStreamEndCapture(s, &graph);
        if (r != FC_OK) { if (graph) (void)hipGraphDestroy(graph); return r; }
        if (e != hipSuccess) return fail(FC_E_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
        hipGraphExec_t exec = nullptr;
        FC_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        FC_HIP(hipGraphDestroy(graph));
        it = ig.graphs.emplace(key, exec).first;
    }
    *out = it->second;
    return FC_OK;
}

// the part of a key every path fills the same way
static GraphKey graph_key(const CallFrame& f, GraphKey::Kind kind, float cfg_strength, float t_scale) {
    GraphKey k;
    k.kind = kind; k.B = f.B; k.cfg_on = f.cfg_on; k.mask_mode = f.mask_mode; k.has_ids = f.has_ids;
    k.cfg_strength = fbits(cfg_strength); k.t_scale = fbits(t_scale);
    return k;
}

// the forward of one integrator evaluation (the caller sets its input x): B rows and, with CFG, their unguided twins B..2B-1, the
// per-row time from ig.tvec, into ig.v2
static FwdCtx integrator_ctx(const CallFrame& f) {
    const IntegratorState& ig = f.u->ig;
    FwdCtx c;
    c.x_mod = f.B; c.time = ig.tvec; c.ids = f.has_ids ? ig.ids_own : nullptr; c.ids_mod = f.B; c.null_from = f.cfg_on ? f.B : 0;
    c.mask = f.mask_mode ? ig.mask_own : nullptr; c.mask_fuse = f.mask_mode == 1;
    c.out = ig.v2; c.B = f.rows;
    return c;
}

// integrator_ctx for a step of a fixed grid.  pre_on: the conditioning rows of every evaluation are in ig.pre (cond_table): init_conv
// fetches slice *evalc, final_conv advances the counter
static FwdCtx step_ctx(const CallFrame& f, bool pre_on) {
    const fc_unet* u = f.u;
    const IntegratorState& ig = u->ig;
    FwdCtx c = integrator_ctx(f);
    if (pre_on) {
        c.fetch.all = ig.pre_ss; c.fetch.evalc = ig.step + 1; c.fetch.dst = u->plan.ss; c.fetch.n4 = f.rows * u->S / 4;
        c.euler.evalc = ig.step + 1;
    }
    return c;
}

// ---- the RK4 interval -----------------------------------------------------------------------------------------------------------------
// rk4_step (sampling.py:36-48) as every RK4 integrator enqueues it, captured or direct: the interval's time (ode_time_launch), then four
// evaluations, each a forward, what the variant puts behind it, and the kernel that closes the stage -- it stores k and hands the next
// evaluation its state and time -- or, behind the fourth, the interval.  The integrators differ in the variant alone.
struct Rk4Variant {
    enum Eval { Forward, ForwardVjp, ForwardGuideWVjp };   // a forward | + vjp_run | + ode_guide_w_launch at the stage's time + vjp_run
    enum Close { Plain, Guided, Likelihood };              // the kernels of ode.hip that close a stage and the interval
    Eval eval;
    Close close;
    int trows;                                             // rows of the time vector: f.rows, or B where there is no guidance pair
    FwdCtx c;                                              // the forward (and, with vjp_run, the chain's d_out / dx_out)
    const float* q = nullptr;                              // Guided: (dv/dx)^T w of the same forward (exact form), or NULL
    const float* probe = nullptr;                          // Likelihood: eps [n_probes][B][m] ...
    double* a = nullptr;                                   // ... and the accumulators [n_probes][B] the interval adds to
    int n_probes = 1;
};

// The likelihood's chains behind one forward: for k in probe order the data-gradient chain with probe k as output cotangent into slice
// k of ll_g.  The trajectory does not depend on the probe and a chain leaves the forward's saved activations as they are, so K probes
// cost one forward and K chains.  n = B * m: the slices' stride is the call's B, in the probes and in ll_g alike.
static int probe_chains(fc_unet* u, FwdCtx c, const float* probes, int n_probes, int n, hipStream_t s) {
    for (int k = 0; k < n_probes; ++k) {
        c.d_out = probes + (size_t)k * n; c.dx_out = u->ig.ll_g + (size_t)k * n;
        FC_TRY(vjp_run(u, c, s));
    }
    return FC_OK;
}

// The likelihood's buffers for n_probes probes per call (plan lifetime; grown, behind the library stream's work, when a call brings
// more probes than any before).  No captured graph holds them: the likelihood launches directly.
static int ll_reserve(fc_unet* u, int n_probes, hipStream_t s) {
    IntegratorState& ig = u->ig;
    if (n_probes <= ig.ll_k) return FC_OK;
    const size_t m = (size_t)u->cfg.channels * u->H * u->W;
    if (ig.ll_k) FC_HIP(hipStreamSynchronize(s));
    ig.ll_k = 0;
    for (double** b : {&ig.ll_d, &ig.rk_dk, &ig.rk_ak}) ig.drop(b);
    ig.drop(&ig.ll_g);
    FC_TRY(ig.get(&ig.ll_d, (size_t)n_probes * u->maxB * 3, "integrator.likelihood"));
    FC_TRY(ig.get(&ig.ll_g, (size_t)n_probes * u->maxB * m, "integrator.likelihood"));
    ig.ll_k = n_probes;
    return FC_OK;
}

// what the two likelihood entry points check of their probe arguments; `fn` names the entry point
static int check_probes(const char* fn, int n_probes, const double* a_probes_out, const double* stderr_out) {
    if (n_probes < 1 || n_probes > FC_LL_MAX_PROBES)
        return fail(FC_E_ARG, std::string(fn) + ": n_probes must lie in [1, " + std::to_string(FC_LL_MAX_PROBES) + "] (the cap on probes per call)");
    if (!a_probes_out != !stderr_out || (n_probes > 1 && !a_probes_out))
        return fail(FC_E_ARG, std::string(fn) + ": several probes need a_probes_out_dev and stderr_out_dev");
    return FC_OK;
}

static int enqueue_rk4_interval(const CallFrame& f, const Rk4Variant& v, float cfg, float t_scale) {
    fc_unet* u = f.u;
    const IntegratorState& ig = u->ig;
    const int n = f.n, m = f.n / f.B, cf = f.cfg_on ? 1 : 0;
    hipStream_t s = f.s;
    // stage j closes evaluation j at time `tcur` (0: t, 1: t + dt/2, 2: t + dt): k_out = its velocity, the next state y + dt*k (full) or
    // y + dt*k/2, the next time `tsel`.  The fourth evaluation closes the interval.
    const struct { float* k_out; int full, tcur, tsel; } stages[4] = {{ig.k1, 0, 0, 1}, {ig.k2, 0, 1, 1}, {ig.k3, 1, 1, 2}, {nullptr, 0, 2, 0}};
    FwdCtx c = v.c;
    FC_TRY(ode_time_launch(ig.step, ig.ts_dev, t_scale, 1, ig.sc, ig.tvec, v.trows, s));
    for (int j = 0; j < 4; ++j) {
        const auto& st = stages[j];
        const float* x = c.x = j == 0 ? ig.y : ig.xs;      // k1 = f(y, t); k2, k3, k4 at the state the stage before wrote
        FC_TRY(run_plan(u->plan, c, s));
        if (v.eval == Rk4Variant::ForwardGuideWVjp) FC_TRY(ode_guide_w_launch(ig.sc, ig.g_sc, ig.v2, x, ig.g_y, ig.g_keep, ig.g_w, n, st.tcur, s));
        if (v.close == Rk4Variant::Likelihood) {
            FC_TRY(probe_chains(u, c, v.probe, v.n_probes, n, s));
            FC_TRY(j < 3 ? ode_ll_stage_launch(ig.sc, ig.y, ig.xs, st.k_out, ig.v2, ig.ll_g, v.probe, ig.ll_d, j, f.B, m, st.full, st.tsel, t_scale, ig.tvec, v.n_probes, s)
                         : ode_ll_final_launch(ig.sc, ig.y, ig.k1, ig.k2, ig.k3, ig.v2, ig.ll_g, v.probe, ig.ll_d, v.a, f.B, m, v.n_probes, s));
            continue;
        }
        if (v.eval != Rk4Variant::Forward) FC_TRY(vjp_run(u, c, s));
        const Rk4Guide guide{ig.g_sc, x, ig.g_y, ig.g_keep, v.q, st.tcur};
        const Rk4Guide* g = v.close == Rk4Variant::Guided ? &guide : nullptr;
        FC_TRY(j < 3 ? ode_rk4_stage_launch(ig.sc, ig.y, ig.xs, st.k_out, ig.v2, n, cf, cfg, st.full, st.tsel, t_scale, ig.tvec, v.trows, g, s)
                     : ode_rk4_final_launch(ig.sc, ig.y, ig.k1, ig.k2, ig.k3, ig.v2, n, cf, cfg, g, s));
    }
    return FC_OK;
}

// enqueue one step of fc_unet_integrate on `s` (captured into a graph by the caller)
// Legacy Euler without CFG: the step needs nothing outside the plan (fc_unet_integrate publishes the first time)
static bool euler_tail_ok(int method, bool cfg_on) { return method == FC_METHOD_EULER && !cfg_on; }

// Step closing (conv_dev.h FL_STEP): inside a replayed Euler step final_res_block's closing launch also runs final_conv, the update and the
// next evaluation's init_conv and fetches the next conditioning slice -- 68 launches per step instead of 70.  Only where that launch is
// the one the flavour is compiled for (Plan::step_blk: the exclusive dim-32 plan at 4x32x32, no mask conditioning) and the call is the
// legacy Euler sampler without CFG or mask on the conditioning table; everything else keeps the three launches.
// FLOCODER_AMD_STEP_CLOSE=0 does too (read per call: the two forms have different graph keys).
static bool step_close_ok(const CallFrame& f, int method, bool pre_on) {
    const fc_unet* u = f.u;
    const char* e = std::getenv("FLOCODER_AMD_STEP_CLOSE");
    if (e && std::strcmp(e, "0") == 0) return false;
    return euler_tail_ok(method, f.cfg_on) && pre_on && f.mask_mode == 0 && u->plan.step_blk != nullptr && u->S % 4 == 0 &&
           u->S / 4 <= 256 * u->plan.step_gsz;         // (a sample's workgroups copy its conditioning row, one float4 per staging thread)
}

// What such a call puts behind integrator_prologue and cond_table, in front of its first replay: the device block of the step-closing
// launch (the call's pointers and constants, the boundary weights, every sample's base epoch) and the FIRST evaluation's init_conv --
// the existing launch, outside the graph; it also fetches conditioning slice 0.
static int step_close_prologue(const CallFrame& f, float dt_euler, float t_scale, int n_steps) {
    fc_unet* u = f.u;
    const IntegratorState& ig = u->ig;
    StepCloseHdr h;
    h.y = ig.y; h.ts = ig.ts_dev; h.sc = ig.sc; h.tvec = ig.tvec; h.step = ig.step; h.evalc = ig.step + 1;
    h.ss_all = ig.pre_ss; h.ss_dst = u->plan.ss; h.dt = dt_euler; h.t_scale = t_scale;
    h.rows = f.rows; h.S = u->S; h.n_slices = n_steps;
    const float *iw = u->P("init_conv.weight"), *ib = u->R("init_conv.bias");
    FC_TRY(step_close_setup_launch(u->plan.step_blk, h, u->P("final_conv.weight"), u->R("final_conv.bias"), iw, ib, u->plan.step_sync,
                                   u->plan.step_gsz, f.s));
    const FwdCtx c = step_ctx(f, true);
    return init_conv_launch(c.fetch, ig.y, f.B, iw, ib, u->plan.x0.p, f.rows, u->cfg.channels, u->H * u->W, u->cfg.dim, f.s);
}

static int enqueue_step(const CallFrame& f, int method, float cfg, float dt_euler, float t_scale, bool pre_on, bool step_close = false) {
    fc_unet* u = f.u;
    const IntegratorState& ig = u->ig;
    const bool cfg_on = f.cfg_on;
    const int rows = f.rows, n = f.n;
    hipStream_t s = f.s;
    FwdCtx c = step_ctx(f, pre_on);
    if (method == FC_METHOD_RK4) return enqueue_rk4_interval(f, {Rk4Variant::Forward, Rk4Variant::Plain, rows, c}, cfg, t_scale);
    if (euler_tail_ok(method, cfg_on)) {   // the update and the next interval's time ride in final_conv: no launches around the plan
        c.x = ig.y;
        c.euler.y = ig.y; c.euler.dt = dt_euler; c.euler.step = ig.step; c.euler.ts = ig.ts_dev; c.euler.t_scale = t_scale;
        c.euler.sc = ig.sc; c.euler.tvec = ig.tvec; c.euler.rows = rows;
        if (step_close) c.step = u->plan.step_blk;
        return run_plan(u->plan, c, s);
    }
    FC_TRY(ode_time_launch(ig.step, ig.ts_dev, t_scale, 0, ig.sc, ig.tvec, rows, s));
    c.x = ig.y;
    FC_TRY(run_plan(u->plan, c, s));
    return ode_euler_update_launch(ig.y, ig.v2, n, cfg_on, cfg, dt_euler, s);
}

// What a fixed-grid call puts behind its frame's hand-over (fc_unet_integrate, fc_unet_log_likelihood): the time grid's device buffer
// (grows only when a longer grid than ever before arrives; captured graphs hold its address) and the call's grid, counters and state
// copied into the library's own buffers.
static int integrator_prologue(const CallFrame& f, const float* x_dev, const float* ts_host, int n_points) {
    IntegratorState& ig = f.u->ig;
    hipStream_t s = f.s;
    if (n_points + 1 > ig.ts_cap) {
        FC_HIP(hipStreamSynchronize(s));
        if (ig.ts_dev) dev_free(ig.ts_dev);
        ig.ts_cap = n_points < 1024 ? 1024 : n_points + 1;   // + 1: the fused Euler tail reads one entry past the grid after the last step
        FC_TRY(dev_alloc(reinterpret_cast<void**>(&ig.ts_dev), ig.ts_cap * sizeof(float), "integrator.ts"));
        ig.drop_graphs();  // captured graphs hold the old ts pointer
    }
    // pageable source: the runtime stages it before returning, so ts_host may be freed by the caller right away
    FC_HIP(hipMemcpyAsync(ig.ts_dev, ts_host, n_points * sizeof(float), hipMemcpyHostToDevice, s));
    FC_HIP(hipMemsetAsync(ig.step, 0, 2 * sizeof(int), s));   // step counter | evaluation counter
    FC_HIP(hipMemcpyAsync(ig.y, x_dev, f.nbytes, hipMemcpyDeviceToDevice, s));
    return FC_OK;
}

// Conditioning of every evaluation of a fixed-grid call, once, into ig.pre (*pre_on_out: the table is in use; not for a single interval
// or a table beyond 2 GiB).
// `pattern`: the evaluation times of an interval -- FC_METHOD_EULER: t_i; FC_METHOD_RK4: the four stage times; kTimesPair: t_i, t_{i+1}.
static constexpr int kTimesPair = 2;
static_assert(FC_METHOD_EULER == 0 && FC_METHOD_RK4 == 1, "ode_all_times_launch takes the method codes as its pattern");
static int cond_table(const CallFrame& f, int pattern, int n_steps, float t_scale, bool* pre_on_out) {
    fc_unet* u = f.u;
    IntegratorState& ig = u->ig;
    const bool has_ids = f.has_ids, cfg_on = f.cfg_on;
    const int rows = f.rows, B = f.B;
    hipStream_t s = f.s;
    // Conditioning of every evaluation, once: the grid is known, so time MLP / class MLP / FiLM projections of all (evaluation, row)
    // pairs are three launches here instead of three at the head of each forward (44 us of every 1.6 ms step inside the replayed graph:
    // cold weights, latency-bound).  Rows are bit-identical to the per-forward ones (same kernels, same time arithmetic).
    const int n_evals = pattern == FC_METHOD_RK4 ? 4 * n_steps : (pattern == kTimesPair ? 2 * n_steps : n_steps);
    const size_t R = (size_t)n_evals * rows, tvn = ((size_t)n_evals + 3) & ~(size_t)3;
    const size_t need = tvn + R * u->td * 3 + R * u->S;
    const bool pre_on = *pre_on_out = n_steps >= 2 && need * sizeof(float) <= (2ull << 30) && R < (1u << 30) / (unsigned)u->S;
    if (!pre_on) return FC_OK;
    {
        if (need > ig.pre_cap) {
            FC_HIP(hipStreamSynchronize(s));
            if (ig.pre) dev_free(ig.pre);
            ig.pre = nullptr; ig.pre_cap = 0;
            FC_TRY(dev_alloc(reinterpret_cast<void**>(&ig.pre), need * sizeof(float), "integrator.cond_table"));
            ig.pre_cap = need;
            ig.drop_graphs();  // captured graphs hold the old table pointer
        }
        float *tv = ig.pre, *te = tv + tvn, *hh = te + R * u->td, *c1 = hh + R * u->td;
        if (ig.pre_ss != c1 + R * u->td)   // the table moved inside the buffer (another number of evaluations): graphs bake its address
            ig.drop_graphs();
        ig.pre_ss = c1 + R * u->td;
        FC_TRY(ode_all_times_launch(ig.ts_dev, n_steps, pattern, t_scale, tv, s));
        TembArgs ta = u->temb_proto;
        ta.B = (int)R; ta.time = tv; ta.rows_per_eval = rows; ta.class_ids = has_ids ? ig.ids_own : nullptr; ta.class_batch_mod = B;
        ta.null_from = cfg_on ? B : 0; ta.t_out = te;
        FC_TRY(temb_launch(ta, hh, c1, s));
        // every ResnetBlock.mlp (SiLU -> Linear td -> 2*Cout, unet.py:79-82) of every row as ONE GEMM [R x td] . [td x S] on the
        // implicit-GEMM kernel (a 1x1 convolution over R one-pixel "images"): the per-forward VALU kernel re-reads the 4 MB weight
        // matrix for every eight rows (1.7 ms at R = 4096), this takes a tenth of that
        FC_TRY(silu_fwd_launch(te, nullptr, hh, R * u->td, s));
        ConvArgs ca;
        ca.s0.p = hh; ca.s0.C = u->td; ca.Cin = u->td; ca.Cout = u->S; ca.B = (int)R; ca.H = ca.W = ca.Hs = ca.Ws = 1; ca.KS = 1;
        ca.w = u->P("__ss_wt"); ca.bias = u->P("__ss_bias"); ca.out = ig.pre_ss;
        FC_TRY(conv_launch(ca, TILE_AUTO, s));
    }
    return FC_OK;
}

// The n_steps intervals of a fixed-grid call, each enqueued by `step`: direct launches under FLOCODER_AMD_NO_GRAPH, else replays of
// graphs cached under `key` (every field but `steps` filled by the caller).
static int replay_steps(const CallFrame& f, GraphKey key, int n_steps, int evals_per_step, const std::function<int()>& step) {
    fc_unet* u = f.u;
    hipStream_t s = f.s;
    if (no_graph()) {
        for (int i = 0; i < n_steps; ++i) FC_TRY(step());
        return FC_OK;
    }
    {
        // One graph holds SEVERAL consecutive intervals (round 3): the step counter, the time grid and the conditioning slice index all
        // live on the device, so a captured interval is position-independent and k of them in a row are one hipGraphLaunch instead
        // of k (the per-interval form left ~4 % of the trajectory between replays: 64 launches of a 70-node graph).  Capped by node
        // count.
        const int nodes_per_step = (int)u->plan.ops.size() * evals_per_step + 16;
        int per = 6144 / nodes_per_step > 0 ? 6144 / nodes_per_step : 1;
        if (per > 255) per = 255;
        for (int left = n_steps; left > 0;) {
            const int k = left < per ? left : per;
            key.steps = k;
            hipGraphExec_t exec = nullptr;
            FC_TRY(cached_graph(u, key, s, [&] {
                int r = FC_OK;
                for (int j = 0; j < k && r == FC_OK; ++j)
                    r = step();
                return r;
            }, &exec));
            // The FIRST replay of a call waits, on the host, for everything this call has put on the stream in front of it (round 4).  Under
            // AMD_DIRECT_DISPATCH=0 -- the mode the sampler ships with -- ROCm 7.2 submits a graph from the calling thread while the plain
            // launches and copies issued just before it are still queued in the runtime's own submission thread: the replay overtook them.
            // Measured (tools/inflight_distinct.py: five calls with different noise / class ids, one at a time): a call's trajectory ran on
            // the PREVIOUS call's conditioning table (rel-L2 1.6e-2 against the oracle, the same value every time, in two or three calls of
            // five); FLOCODER_AMD_NO_GRAPH=1, AMD_DIRECT_DISPATCH=1 and this wait each give 1e-7 in all of them, an event wait on the
            // same stream does not.  bench.py never saw it: every timed step integrates the same samples, so a stale table is the right
            // one.  Replays that follow a replay are ordered (RK4: five graphs per call); work issued behind a replay is ordered as well.
            // Cost: the host idles for the prologue (~0.1 ms per call of 80 ms).
            if (left == n_steps) FC_HIP(hipStreamSynchronize(s));
            FC_HIP(hipGraphLaunch(exec, s));
            left -= k;
        }
    }
    return FC_OK;
}

int fc_unet_integrate(fc_unet* u, int method, float* x_dev, int B, int H, int W, const float* ts_host, int n_points, float dt_euler,
                      float t_scale, const int64_t* ids, float cfg_strength, const float* mask, int mask_is_ones, void* stream) {
    if (!u || !x_dev || !ts_host || B < 1 || n_points < 1) return fail(FC_E_ARG, "fc_unet_integrate: bad argument");
    if (method != FC_METHOD_EULER && method != FC_METHOD_RK4) return fail(FC_E_ARG, "fc_unet_integrate: unknown method");
    CallFrame f;
    FC_TRY(f.begin(u, B, H, W, ids, cfg_strength, mask, mask_is_ones, stream));
    FC_TRY(f.enter());
    IntegratorState& ig = u->ig;
    const bool cfg_on = f.cfg_on;
    const int rows = f.rows, n_steps = method == FC_METHOD_RK4 ? n_points - 1 : n_points;
    hipStream_t s = f.s;
    FC_TRY(integrator_prologue(f, x_dev, ts_host, n_points));
    bool pre_on = false;
    FC_TRY(cond_table(f, method, n_steps, t_scale, &pre_on));
    if (euler_tail_ok(method, cfg_on))   // time of the first interval; every step publishes its successor's
        FC_TRY(ode_time_launch(ig.step, ig.ts_dev, t_scale, 0, ig.sc, ig.tvec, rows, s));
    GraphKey key = graph_key(f, method == FC_METHOD_RK4 ? GraphKey::Rk4 : GraphKey::Euler, cfg_strength, t_scale);
    key.pre_on = pre_on; key.dt_euler = fbits(dt_euler);
    const bool step_close = key.step_close = step_close_ok(f, method, pre_on);
    if (step_close) FC_TRY(step_close_prologue(f, dt_euler, t_scale, n_steps));
    FC_TRY(replay_steps(f, key, n_steps, method == FC_METHOD_RK4 ? 4 : 1,
                        [&] { return enqueue_step(f, method, cfg_strength, dt_euler, t_scale, pre_on, step_close); }));
    return f.finish(x_dev);
}

// ---- likelihood / inversion on the RK4 grid ------------------------------------------------------------------------------------------
// x from ts[0] to ts[n_points-1] with rk4_step on the caller's grid (log p needs it walked from t = 1 to t = 0), every evaluation a
// training-mode forward followed by the backward plan's data-gradient chain with the probe as output cotangent (vjp_run), the stage
// kernels of ode.hip carrying a[b] = integral of eps^T (dv/dx) eps dt.  The grid is known, so nothing is decided on the host: the call
// returns with the whole loop queued.  Direct launches (4 (n_points - 1) forwards + chains); the arena ends up holding the last stage's
// forward, which belongs to nobody: the serial moves and a later backward re-runs its own forward.
// K probes (fc_unet_log_likelihood_probes; K = 1 without per-probe outputs is fc_unet_log_likelihood): one forward per evaluation, K
// chains behind it, every probe its own accumulator a_k in a_probes_out; a_out is their mean and logp is formed from it.
static int log_likelihood_rk4(const char* fn, fc_unet* u, float* x_dev, int B, int H, int W, const float* ts_host, int n_points, float t_scale,
                              const int64_t* ids, const float* mask, int mask_is_ones, const float* probes_dev, int n_probes,
                              double* a_out_dev, double* logp_out_dev, double* a_probes_out_dev, double* stderr_out_dev, void* stream) {
    if (!u || !x_dev || !ts_host || !probes_dev || !a_out_dev || !logp_out_dev || B < 1) return fail(FC_E_ARG, std::string(fn) + ": null argument");
    if (n_points < 2) return fail(FC_E_ARG, std::string(fn) + ": the time grid needs at least two points");
    FC_TRY(check_probes(fn, n_probes, a_probes_out_dev, stderr_out_dev));
    FC_TRY(check_aligned16({probes_dev}, (std::string(fn) + ": probe_dev must be 16-byte aligned (the kernels read it as float4)").c_str()));
    CallFrame f;
    FC_TRY(f.begin(u, B, H, W, ids, 0.0f, mask, mask_is_ones, stream));      // no guidance
    if (!u->keep_all) return fail(FC_E_STATE, std::string(fn) + ": no backward plan for this shape; call fc_unet_train_reserve");
    FC_TRY(vjp_check(u, B, H, W, fn));
    IntegratorState& ig = u->ig;
    const int m = u->cfg.channels * H * W;
    FC_TRY(ll_reserve(u, n_probes, f.s));
    FC_TRY(f.enter());
    FC_TRY(integrator_prologue(f, x_dev, ts_host, n_points));
    double* acc = a_probes_out_dev ? a_probes_out_dev : a_out_dev;           // one probe without per-probe outputs: a is its accumulator
    FC_HIP(hipMemsetAsync(acc, 0, (size_t)n_probes * B * sizeof(double), f.s));
    Rk4Variant v{Rk4Variant::ForwardVjp, Rk4Variant::Likelihood, B, integrator_ctx(f)};   // v2 = v(x, tvec), ll_g[k] = (dv/dx)^T probe k
    v.probe = probes_dev; v.a = acc; v.n_probes = n_probes;
    for (int i = 0; i + 1 < n_points; ++i) FC_TRY(enqueue_rk4_interval(f, v, 0.0f, t_scale));
    if (a_probes_out_dev) FC_TRY(ode_ll_mean_launch(a_probes_out_dev, n_probes, B, a_out_dev, stderr_out_dev, 0, f.s));
    FC_TRY(ode_ll_logp_launch(ig.y, a_out_dev, logp_out_dev, B, m, f.s));
    return f.finish(x_dev);
}

int fc_unet_log_likelihood(fc_unet* u, float* x_dev, int B, int H, int W, const float* ts_host, int n_points, float t_scale,
                           const int64_t* ids, const float* mask, int mask_is_ones, const float* probe_dev, double* a_out_dev,
                           double* logp_out_dev, void* stream) {
    return log_likelihood_rk4("fc_unet_log_likelihood", u, x_dev, B, H, W, ts_host, n_points, t_scale, ids, mask, mask_is_ones, probe_dev, 1,
                              a_out_dev, logp_out_dev, nullptr, nullptr, stream);
}

int fc_unet_log_likelihood_probes(fc_unet* u, float* x_dev, int B, int H, int W, const float* ts_host, int n_points, float t_scale,
                                  const int64_t* ids, const float* mask, int mask_is_ones, const float* probes_dev, int n_probes,
                                  double* a_out_dev, double* logp_out_dev, double* a_probes_out_dev, double* stderr_out_dev, void* stream) {
    if (!a_probes_out_dev || !stderr_out_dev) return fail(FC_E_ARG, "fc_unet_log_likelihood_probes: null argument");
    return log_likelihood_rk4("fc_unet_log_likelihood_probes", u, x_dev, B, H, W, ts_host, n_points, t_scale, ids, mask, mask_is_ones,
                              probes_dev, n_probes, a_out_dev, logp_out_dev, a_probes_out_dev, stderr_out_dev, stream);
}

int fc_debug_probe_dot(const float* probe_dev, const float* g_dev, double* out_dev, int batch, int64_t per_sample, void* stream) {
    if (!probe_dev || !g_dev || !out_dev) return fail(FC_E_ARG, "fc_debug_probe_dot: null argument");
    FC_TRY(check_aligned16({probe_dev, g_dev}, "fc_debug_probe_dot: inputs must be 16-byte aligned (read as float4)"));
    if (per_sample < 1 || per_sample > 0x7fffffff) return fail(FC_E_SHAPE, "fc_debug_probe_dot: bad element count");
    return ode_ll_dot_launch(probe_dev, g_dev, out_dev, nullptr, batch, (int)per_sample, 1, static_cast<hipStream_t>(stream));
}

// ---- measurement guidance on the RK4 grid ------------------------------------------------------------------------------------------
// fc_unet_integrate_guided: fc_unet_integrate(FC_METHOD_RK4) with every stage velocity corrected towards the measurement (ode.hip).
// sigma_y^2 and gamma reach the kernels through a device scalar block (ig.g_sc), not as kernel arguments: a captured interval then
// serves every (sigma_y, gamma) -- a caller tuning them replays one graph instead of capturing one per value -- and the key of a guided
// graph is the key of the plain one plus its kind.
static int alloc_guided(fc_unet* u, bool exact) {
    IntegratorState& ig = u->ig;
    const size_t nstate = (size_t)u->maxB * u->cfg.channels * u->H * u->W;
    const char* tag = "integrator.guided";
    if (!ig.g_sc) {
        FC_TRY(ig.get(&ig.g_y, nstate, tag));
        FC_TRY(ig.get(&ig.g_keep, nstate, tag));
        FC_TRY(ig.get(&ig.g_sc, 4, tag));            // last: a first call that failed half-way allocates again
        ig.drop_graphs();
    }
    if (exact && !ig.g_q) {
        FC_TRY(ig.get(&ig.g_w, nstate, tag));
        FC_TRY(ig.get(&ig.g_q, nstate, tag));
        ig.drop_graphs();
    }
    return FC_OK;
}

int fc_unet_integrate_guided(fc_unet* u, float* x_dev, int B, int H, int W, const float* ts_host, int n_points, float t_scale,
                             const int64_t* ids, float cfg_strength, const float* mask, int mask_is_ones, const float* y_meas,
                             const float* keep, float sigma_y, float gamma, int jacobian, void* stream) {
    if (!u || !x_dev || !ts_host || !y_meas || !keep || B < 1) return fail(FC_E_ARG, "fc_unet_integrate_guided: null argument");
    if (n_points < 2) return fail(FC_E_ARG, "fc_unet_integrate_guided: the time grid needs at least two points");
    if (jacobian != FC_JACOBIAN_IDENTITY && jacobian != FC_JACOBIAN_EXACT) return fail(FC_E_ARG, "fc_unet_integrate_guided: unknown jacobian mode");
    for (int i = 0; i < n_points; ++i)
        if (!(ts_host[i] > 0.0f)) return fail(FC_E_ARG, "fc_unet_integrate_guided: every grid point must be > 0 (the correction is gamma (1-t)/t g)");
    if (!(sigma_y >= 0.0f)) return fail(FC_E_ARG, "fc_unet_integrate_guided: sigma_y must be >= 0");
    if (!std::isfinite(gamma)) return fail(FC_E_ARG, "fc_unet_integrate_guided: gamma must be finite");
    FC_TRY(check_aligned16({x_dev, y_meas, keep}, "fc_unet_integrate_guided: x, measurement and keep must be 16-byte aligned (the kernels read them as float4)"));
    const bool exact = jacobian == FC_JACOBIAN_EXACT;
    CallFrame f;
    FC_TRY(f.begin(u, B, H, W, ids, cfg_strength, mask, mask_is_ones, stream));
    if (exact) {
        if (f.cfg_on)
            return fail(FC_E_ARG, "fc_unet_integrate_guided: the exact Jacobian takes no classifier-free guidance (the chain differentiates one "
                                  "forward, not the guided pair)");
        if (!u->keep_all) return fail(FC_E_STATE, "fc_unet_integrate_guided: no backward plan for this shape; call fc_unet_train_reserve");
        FC_TRY(vjp_check(u, B, H, W, "fc_unet_integrate_guided"));
    }
    IntegratorState& ig = u->ig;
    FC_TRY(alloc_guided(u, exact));
    const int n_steps = n_points - 1;
    hipStream_t s = f.s;
    FC_TRY(f.enter());
    FC_TRY(integrator_prologue(f, x_dev, ts_host, n_points));
    FC_HIP(hipMemcpyAsync(ig.g_y, y_meas, f.nbytes, hipMemcpyDeviceToDevice, s));
    FC_HIP(hipMemcpyAsync(ig.g_keep, keep, f.nbytes, hipMemcpyDeviceToDevice, s));
    const float gsc[4] = {(float)((double)sigma_y * (double)sigma_y), gamma, 0.f, 0.f};
    FC_HIP(hipMemcpyAsync(ig.g_sc, gsc, sizeof(gsc), hipMemcpyHostToDevice, s));   // pageable source: staged before the call returns
    if (!exact) {   // fc_unet_integrate's captured RK4 interval with the guided stage kernels
        bool pre_on = false;
        FC_TRY(cond_table(f, FC_METHOD_RK4, n_steps, t_scale, &pre_on));
        GraphKey key = graph_key(f, GraphKey::Rk4Guided, cfg_strength, t_scale);
        key.pre_on = pre_on;
        const Rk4Variant v{Rk4Variant::Forward, Rk4Variant::Guided, f.rows, step_ctx(f, pre_on)};
        FC_TRY(replay_steps(f, key, n_steps, 4, [&] { return enqueue_rk4_interval(f, v, cfg_strength, t_scale); }));
    } else {
        // the likelihood's structure: every evaluation a training-form forward, w, the data-gradient chain with w as output cotangent,
        // then the stage kernel with q = (dv/dx)^T w; direct launches, nothing decided on the host
        Rk4Variant v{Rk4Variant::ForwardGuideWVjp, Rk4Variant::Guided, B, integrator_ctx(f)};
        v.c.d_out = ig.g_w; v.q = v.c.dx_out = ig.g_q;
        for (int i = 0; i < n_steps; ++i) FC_TRY(enqueue_rk4_interval(f, v, 0.0f, t_scale));
    }
    return f.finish(x_dev);
}

int fc_ode_guided_correct(const float* v_dev, const float* x_dev, const float* y_dev, const float* a_dev, int64_t n, float t, float sigma_y,
                          float gamma, float* out_dev, void* stream) {
    if (!v_dev || !x_dev || !y_dev || !a_dev || !out_dev) return fail(FC_E_ARG, "fc_ode_guided_correct: null argument");
    FC_TRY(check_aligned16({v_dev, x_dev, y_dev, a_dev, out_dev}, "fc_ode_guided_correct: tensors must be 16-byte aligned (read as float4)"));
    if (!(t > 0.0f)) return fail(FC_E_ARG, "fc_ode_guided_correct: t must be > 0");
    if (!(sigma_y >= 0.0f)) return fail(FC_E_ARG, "fc_ode_guided_correct: sigma_y must be >= 0");
    if (n < 1 || n > 0x7fffffff) return fail(FC_E_SHAPE, "fc_ode_guided_correct: bad element count");
    return ode_guided_correct_launch(v_dev, x_dev, y_dev, a_dev, out_dev, (int)n, t, (float)((double)sigma_y * (double)sigma_y), gamma,
                                     static_cast<hipStream_t>(stream));
}

int fc_debug_unet_guided_buffers(const fc_unet* u, const float** stage_x, const float** stage_time, const float** w, const float** q) {
    if (!u || !u->ig.g_q) return fail(FC_E_STATE, "fc_debug_unet_guided_buffers: no exact-form guided call on the current plan");
    if (stage_x) *stage_x = u->ig.xs;
    if (stage_time) *stage_time = u->ig.tvec;
    if (w) *w = u->ig.g_w;
    if (q) *q = u->ig.g_q;
    return FC_OK;
}

// ---- stochastic sampling on a fixed grid ---------------------------------------------------------------------------------------------
// fc_unet_integrate_sde: fc_unet_integrate's frame with ode.hip's SDE update behind each forward.  An interval is ode_time_launch (opens
// the interval: scaled time rows of t_i, the counter moves), the plan, the update -- the launch structure of the Euler step with guidance;
// Heun adds a second plan run and update.  The seed, the noise pointer and the sample ids reach the kernel through device memory
// (ig.sde_prm, ig.sde_ids), so the key of a captured interval carries the scheme, sigma's bits and the noise source and nothing of the call.
static int alloc_sde(fc_unet* u) {
    IntegratorState& ig = u->ig;
    if (ig.sde_prm) return FC_OK;
    FC_TRY(ig.get(&ig.sde_ids, (size_t)u->maxB, "integrator.sde"));
    return ig.get(&ig.sde_prm, 1, "integrator.sde");       // last: a first call that failed half-way allocates again
}

static int enqueue_sde_step(const CallFrame& f, int scheme, float cfg, float sigma, int use_noise, float t_scale, bool pre_on) {
    fc_unet* u = f.u;
    const IntegratorState& ig = u->ig;
    const int rows = f.rows, n = f.n, m = f.n / f.B, cf = f.cfg_on ? 1 : 0;
    hipStream_t s = f.s;
    FwdCtx c = step_ctx(f, pre_on);
    FC_TRY(ode_time_launch(ig.step, ig.ts_dev, t_scale, 1, ig.sc, ig.tvec, rows, s));
    c.x = ig.y;
    FC_TRY(run_plan(u->plan, c, s));                                                                                     // v(y, t_i)
    if (scheme == FC_SDE_EULER_MARUYAMA)
        return ode_sde_update_launch(ig.step, ig.ts_dev, ig.sde_prm, ig.sde_ids, ig.y, ig.xs, ig.k1, ig.v2, n, m, cf, cfg, sigma, 0, use_noise,
                                     t_scale, ig.tvec, rows, s);
    FC_TRY(ode_sde_update_launch(ig.step, ig.ts_dev, ig.sde_prm, ig.sde_ids, ig.y, ig.xs, ig.k1, ig.v2, n, m, cf, cfg, sigma, 1, use_noise,
                                 t_scale, ig.tvec, rows, s));                                                            // predictor, t_{i+1}
    c.x = ig.xs;
    FC_TRY(run_plan(u->plan, c, s));                                                                                     // v(xs, t_{i+1})
    return ode_sde_update_launch(ig.step, ig.ts_dev, ig.sde_prm, ig.sde_ids, ig.y, ig.xs, ig.k1, ig.v2, n, m, cf, cfg, sigma, 2, use_noise,
                                 t_scale, ig.tvec, rows, s);
}

int fc_unet_integrate_sde(fc_unet* u, int scheme, float* x_dev, int B, int H, int W, const float* ts_host, int n_points, float t_scale,
                          const int64_t* ids, float cfg_strength, const float* mask, int mask_is_ones, float sigma, uint64_t seed,
                          const int64_t* sample_ids, const float* noise, void* stream) {
    if (!u || !x_dev || !ts_host || B < 1) return fail(FC_E_ARG, "fc_unet_integrate_sde: null argument");
    if (scheme != FC_SDE_EULER_MARUYAMA && scheme != FC_SDE_HEUN) return fail(FC_E_ARG, "fc_unet_integrate_sde: unknown scheme");
    if (n_points < 2) return fail(FC_E_ARG, "fc_unet_integrate_sde: the time grid needs at least two points");
    for (int i = 0; i < n_points; ++i)
        if (!(ts_host[i] >= 0.0f && ts_host[i] <= 1.0f) || (i > 0 && ts_host[i] < ts_host[i - 1]))
            return fail(FC_E_ARG, "fc_unet_integrate_sde: the grid must be non-decreasing within [0, 1] (the diffusion is sigma sqrt(1-t))");
    if (!(sigma >= 0.0f) || !std::isfinite(sigma)) return fail(FC_E_ARG, "fc_unet_integrate_sde: sigma must be finite and >= 0");
    FC_TRY(check_aligned16({x_dev, noise}, "fc_unet_integrate_sde: x and the noise must be 16-byte aligned (the kernels read them as float4)"));
    CallFrame f;
    FC_TRY(f.begin(u, B, H, W, ids, cfg_strength, mask, mask_is_ones, stream));
    IntegratorState& ig = u->ig;
    FC_TRY(alloc_sde(u));
    const int n_steps = n_points - 1, use_noise = noise ? 1 : 0, heun = scheme == FC_SDE_HEUN;
    hipStream_t s = f.s;
    FC_TRY(f.enter());
    FC_TRY(integrator_prologue(f, x_dev, ts_host, n_points));
    const SdeParams prm{seed, noise};
    FC_HIP(hipMemcpyAsync(ig.sde_prm, &prm, sizeof(prm), hipMemcpyHostToDevice, s));   // pageable source: staged before the call returns
    if (sample_ids) FC_HIP(hipMemcpyAsync(ig.sde_ids, sample_ids, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    else FC_TRY(ode_iota_launch(ig.sde_ids, B, s));
    bool pre_on = false;
    FC_TRY(cond_table(f, heun ? kTimesPair : FC_METHOD_EULER, n_steps, t_scale, &pre_on));
    GraphKey key = graph_key(f, GraphKey::Sde, cfg_strength, t_scale);
    key.pre_on = pre_on; key.sde_scheme = scheme; key.sde_noise = use_noise; key.sde_sigma = fbits(sigma);
    FC_TRY(replay_steps(f, key, n_steps, heun ? 2 : 1,
                        [&] { return enqueue_sde_step(f, scheme, cfg_strength, sigma, use_noise, t_scale, pre_on); }));
    return f.finish(x_dev);
}

int fc_ode_normal_field(float* out_dev, uint64_t seed, int64_t draw_index, const int64_t* sample_ids_dev, int batch, int64_t per_sample,
                        void* stream) {
    if (!out_dev) return fail(FC_E_ARG, "fc_ode_normal_field: null argument");
    FC_TRY(check_aligned16({out_dev}, "fc_ode_normal_field: out must be 16-byte aligned (written as float4)"));
    if (draw_index < 0 || draw_index > 0xffffffffLL) return fail(FC_E_ARG, "fc_ode_normal_field: the draw index is a 32-bit counter word");
    if (batch < 1 || per_sample < 4 || (per_sample & 3) || (long long)batch * per_sample > 0x7fffffffLL)
        return fail(FC_E_SHAPE, "fc_ode_normal_field: elements per sample must be a positive multiple of 4, batch * per_sample < 2^31");
    return ode_normal_field_launch(out_dev, seed, (unsigned)draw_index, sample_ids_dev, batch * (int)per_sample, (int)per_sample,
                                   static_cast<hipStream_t>(stream));
}

// ---- adaptive RK45 ----------------------------------------------------------------------------------------------------------------
// Both modes run ode.hip's grouped kernels: the batch-coupled solve is one controller over all B*C*H*W unknowns, the per-sample solve
// one controller per sample.  Each mode keeps the partition it was introduced with -- it fixes the summation order of the norms and
// with it the bits: coupled, one workgroup per 1024 unknowns of the batch, at most 2048 (the elementwise grid of ode.hip); per sample,
// at most 64, so that a sample's step sequence depends on C*H*W alone, not on the batch size.
static constexpr int kRk45MaxAttempts = 10000;     // a field that never settles raises instead of spinning (scipy has no such cap)
static constexpr int kRk45CoupledChunks = 2048, kRk45PerSampleChunks = 64;

static Rk45Groups rk45_groups(const fc_unet* u, int B, bool per_sample) {
    const int m = u->cfg.channels * u->H * u->W;
    return per_sample ? Rk45Groups{B, 1, m, rk45_chunks(m, kRk45PerSampleChunks)}
                      : Rk45Groups{1, B, B * m, rk45_chunks(B * m, kRk45CoupledChunks)};
}

// The controller state, allocated by the first RK45 call (plan lifetime) so handles that never use it keep their footprint; the
// partial sums fit either mode's partition.
static int alloc_rk45(fc_unet* u) {
    IntegratorState& ig = u->ig;
    const size_t nstate = (size_t)u->maxB * u->cfg.channels * u->H * u->W;
    const char* tag = "integrator.rk45";
    const Rk45Groups cg = rk45_groups(u, u->maxB, false), pg = rk45_groups(u, u->maxB, true);
    const size_t parts = std::max((size_t)cg.G * cg.chunks, (size_t)pg.G * pg.chunks);
    FC_TRY(ig.get(&ig.rk_y, nstate, tag));
    FC_TRY(ig.get(&ig.rk_ynew, nstate, tag));
    for (int j = 0; j < 7; ++j) FC_TRY(ig.get(&ig.rk_k.k[j], nstate, tag));
    FC_TRY(ig.get(&ig.rk_part, 2 * parts, tag));
    FC_TRY(ig.get(&ig.rk_sum, 1, tag));
    return ig.get(&ig.rk_st, u->maxB, tag);       // last: a first call that failed half-way allocates again
}

// What the adaptive likelihood adds to the controller state (plan lifetime, first use): the divergence track a | a_new and the seven
// rows of its K values; g of the running evaluation is the RK4 likelihood's buffer.
static int alloc_rk45_ll(fc_unet* u, int n_probes, bool per_probe, hipStream_t s) {
    IntegratorState& ig = u->ig;
    FC_TRY(ll_reserve(u, n_probes, s));
    if (per_probe && !ig.rk_dk) {   // (ll_reserve drops them when the probe count grows)
        FC_TRY(ig.get(&ig.rk_dk, (size_t)7 * ig.ll_k * u->maxB, "integrator.rk45_likelihood"));
        FC_TRY(ig.get(&ig.rk_ak, (size_t)ig.ll_k * u->maxB, "integrator.rk45_likelihood"));
    }
    if (ig.rk_a) return FC_OK;
    FC_TRY(ig.get(&ig.rk_d, (size_t)u->maxB * 7, "integrator.rk45_likelihood"));
    return ig.get(&ig.rk_a, (size_t)u->maxB * 2, "integrator.rk45_likelihood");
}

// The likelihood side of an adaptive solve (fc_unet_log_likelihood_rk45): every evaluation is the forward, the data-gradient chain with
// the probe as output cotangent and the per-row reduction d = sum eps g into row `slot` of the divergence track's K values.
// n_probes probes ([K][B][m]): d is their mean; with a_probes_out / stderr_out every probe's own integral is carried beside it.
struct Rk45Likelihood { const float* probe; double *a_out, *logp_out; int n_probes; double *a_probes_out, *stderr_out; };

// one attempt of RungeKutta._step_impl for every group that still steps: five stages, y_new and f(t + h, y_new), the error norms,
// the controllers, with a dense-output request (`ev`) the frames an accepted step serves, the commit, the status summary
// `eval(slot)`: the evaluation that yields K_slot
static int enqueue_rk45_attempt(fc_unet* u, const Rk45Groups& g, const std::function<int(int)>& eval, int cf, float cfg, float t_scale,
                                const Rk45Eval* ev, const Rk45LL* ll, hipStream_t s) {
    const IntegratorState& ig = u->ig;
    for (int st = 1; st <= 5; ++st) {
        FC_TRY(rk45_stage_launch(g, ig.rk_st, st, ig.rk_y, ig.rk_k, ig.v2, cf, cfg, ig.xs, t_scale, ig.tvec, s));
        FC_TRY(eval(st));                                                                                     // K_st
    }
    FC_TRY(rk45_finish_launch(g, ig.rk_st, ig.rk_y, ig.rk_ynew, ig.rk_k, ig.v2, cf, cfg, ig.xs, t_scale, ig.tvec, s));
    FC_TRY(eval(6));                                                                                          // f(t + h, y_new)
    FC_TRY(rk45_error_launch(g, ig.rk_st, ig.rk_y, ig.rk_ynew, ig.rk_k, ig.v2, cf, cfg, ig.rk_part, s));
    FC_TRY(rk45_control_launch(g, ig.rk_st, ig.rk_part, ev, ll, s));
    if (ev) FC_TRY(rk45_dense_launch(g, ig.rk_st, ev, ig.rk_y, ig.rk_k, s));       // reads y and K0..K6 before the commit replaces them
    FC_TRY(rk45_commit_launch(g, ig.rk_st, ig.rk_y, ig.rk_ynew, ig.rk_k.k[0], ig.rk_k.k[6], s));
    return rk45_status_launch(g, ig.rk_st, ig.rk_sum, s);
}

// solve_ivp's checks of t_eval, with its messages
static int check_t_eval(const char* fn, const double* te, int n_eval, double t0, double t1) {
    const double lo = std::min(t0, t1), hi = std::max(t0, t1);
    for (int j = 0; j < n_eval; ++j)
        if (!(te[j] >= lo && te[j] <= hi)) return fail(FC_E_ARG, std::string(fn) + ": Values in `t_eval` are not within `t_span`.");
    for (int j = 1; j < n_eval; ++j) {
        const double d = te[j] - te[j - 1];
        if ((t1 > t0 && d <= 0) || (t1 < t0 && d >= 0))
            return fail(FC_E_ARG, std::string(fn) + ": Values in `t_eval` are not properly sorted.");
    }
    return FC_OK;
}

// The dense-output request of this call in the handle's device record (header, then the times), ahead of the solve on `s`.  The record
// grows only when a call brings more times than any before; captured attempts bake its address.
static int stage_rk45_eval(fc_unet* u, const double* te, int n_eval, float* frames_dev, hipStream_t s) {
    IntegratorState& ig = u->ig;
    if (n_eval > ig.rk_ev_cap) {
        FC_HIP(hipStreamSynchronize(s));
        if (ig.rk_ev) dev_free(ig.rk_ev);
        ig.rk_ev = nullptr; ig.rk_ev_cap = 0;
        const int cap = n_eval < 1024 ? 1024 : n_eval;
        FC_TRY(dev_alloc(reinterpret_cast<void**>(&ig.rk_ev), sizeof(Rk45Eval) + (size_t)cap * sizeof(double), "integrator.rk45_eval"));
        ig.rk_ev_cap = cap;
        ig.drop_graphs();
    }
    std::vector<unsigned char> rec(sizeof(Rk45Eval) + (size_t)n_eval * sizeof(double));
    const Rk45Eval head{frames_dev, n_eval, 0};
    std::memcpy(rec.data(), &head, sizeof(head));
    std::memcpy(rec.data() + sizeof(head), te, (size_t)n_eval * sizeof(double));
    // pageable source: the runtime stages it before returning (as the time grid of fc_unet_integrate)
    FC_HIP(hipMemcpyAsync(ig.rk_ev, rec.data(), rec.size(), hipMemcpyHostToDevice, s));
    return FC_OK;
}

// fc_unet_integrate_rk45 (per_sample = false), fc_unet_integrate_rk45_per_sample, with n_eval > 0 fc_unet_integrate_rk45_dense, and with
// `lk` fc_unet_log_likelihood_rk45: the same solve over the augmented state [x, a] (ode.hip), every evaluation the training-form forward
// with the data-gradient chain behind it, launched directly; `fn` names the entry point in argument errors
static int integrate_rk45(fc_unet* u, bool per_sample, const char* fn, float* x_dev, int B, int H, int W, double t0, double t1,
                          double rtol, double atol, float t_scale, const int64_t* ids, float cfg_strength, const float* mask,
                          int mask_is_ones, const double* t_eval, int n_eval, float* frames_dev, int* counters, void* stream,
                          const Rk45Likelihood* lk = nullptr) {
    if (!u || !x_dev || !counters || B < 1) return fail(FC_E_ARG, std::string(fn) + ": bad argument");
    if (n_eval < 0 || (n_eval > 0 && (!t_eval || !frames_dev || (reinterpret_cast<uintptr_t>(frames_dev) & 15))))
        return fail(FC_E_ARG, std::string(fn) + ": t_eval needs its times and a 16-byte aligned frames buffer");
    if (!(atol >= 0)) return fail(FC_E_ARG, std::string(fn) + ": `atol` must be positive.");      // validate_tol
    if (!std::isfinite(t0) || !std::isfinite(t1)) return fail(FC_E_ARG, std::string(fn) + ": t0 and t1 must be finite");
    const double eps100 = 100 * 2.220446049250313e-16;
    if (rtol < eps100) rtol = eps100;                                                                         // validate_tol (host warns)
    FC_TRY(check_t_eval(fn, t_eval, n_eval, t0, t1));
    CallFrame f;
    FC_TRY(f.begin(u, B, H, W, ids, cfg_strength, mask, mask_is_ones, stream));
    IntegratorState& ig = u->ig;
    if (lk) {
        if (!u->keep_all) return fail(FC_E_STATE, std::string(fn) + ": no backward plan for this shape; call fc_unet_train_reserve");
        FC_TRY(vjp_check(u, B, H, W, fn));
    }
    const Rk45Groups g = rk45_groups(u, B, per_sample);
    for (int i = 0; i < g.G; ++i) { counters[3 * i] = 1; counters[3 * i + 1] = counters[3 * i + 2] = 0; }   // nfev, accepted, rejected
    const int n = f.n, cf = f.cfg_on ? 1 : 0;
    hipStream_t s = f.s;
    if (t0 == t1) {                              // scipy: one evaluation, no step, y0 returned; every requested time is t0
        for (int j = 0; j < n_eval; ++j) FC_HIP(hipMemcpyAsync(frames_dev + (size_t)j * n, x_dev, f.nbytes, hipMemcpyDeviceToDevice, f.caller));
        return FC_OK;
    }
    if (!ig.rk_st) FC_TRY(alloc_rk45(u));
    if (lk) FC_TRY(alloc_rk45_ll(u, lk->n_probes, lk->a_probes_out != nullptr, s));
    if (!ig.rk_host) { void* hp = nullptr; FC_HIP(hipHostMalloc(&hp, sizeof(Rk45Status), hipHostMallocDefault)); ig.rk_host = static_cast<Rk45Status*>(hp); }
    if (!ig.ev_rk) FC_HIP(hipEventCreateWithFlags(&ig.ev_rk, hipEventDisableTiming));

    FC_TRY(f.enter());
    if (n_eval > 0) FC_TRY(stage_rk45_eval(u, t_eval, n_eval, frames_dev, s));
    const Rk45Eval* ev = n_eval > 0 ? ig.rk_ev : nullptr;

    // f(t0, y0) and select_initial_step of every group (two forwards, no graph)
    FwdCtx c = integrator_ctx(f);
    c.x = ig.xs;   // every forward of the solve reads the stage input the RK45 kernels write
    const int K = lk ? lk->n_probes : 1;
    const bool per_probe = lk && lk->a_probes_out;
    const Rk45LL track{ig.rk_a, ig.rk_d, B, K, per_probe ? ig.rk_dk : nullptr, per_probe ? ig.rk_ak : nullptr};
    const Rk45LL* ll = lk ? &track : nullptr;
    const int m1 = n / B;
    if (lk) {      // v2 = v(xs, tvec), ll_g[k] = (dv/dx)^T probe k; a = 0 (and every a_k = 0) at t0
        FC_HIP(hipMemsetAsync(ig.rk_a, 0, (size_t)2 * B * sizeof(double), s));
        if (per_probe) FC_HIP(hipMemsetAsync(ig.rk_ak, 0, (size_t)K * B * sizeof(double), s));
    }
    const std::function<int(int)> eval = [&](int slot) {
        FC_TRY(run_plan(u->plan, c, s));
        if (!lk) return (int)FC_OK;
        FC_TRY(probe_chains(u, c, lk->probe, K, n, s));
        return ode_ll_dot_launch(lk->probe, ig.ll_g, ig.rk_d + (size_t)slot * B, per_probe ? ig.rk_dk + (size_t)slot * K * B : nullptr, B, m1, K, s);
    };
    FC_TRY(rk45_setup_launch(g, x_dev, ig.rk_y, ig.xs, ig.rk_st, t0, t1, rtol, atol, kRk45MaxAttempts, t_scale, ig.tvec, cf, s));
    FC_TRY(eval(0));                                                                                          // f0
    FC_TRY(rk45_d01_launch(g, ig.rk_st, ig.rk_y, ig.rk_k.k[0], ig.v2, cf, cfg_strength, ig.rk_part, s));
    FC_TRY(rk45_h0_launch(g, ig.rk_st, ig.rk_part, t_scale, ig.tvec, cf, ll, s));
    FC_TRY(rk45_y1_launch(g, ig.rk_st, ig.rk_y, ig.rk_k.k[0], ig.xs, s));
    FC_TRY(eval(1));                                                                                          // f(t0 + h0, y0 + h0 f0)
    FC_TRY(rk45_d2_launch(g, ig.rk_st, ig.rk_y, ig.rk_k.k[0], ig.v2, cf, cfg_strength, ig.rk_part, s));
    FC_TRY(rk45_h1_launch(g, ig.rk_st, ig.rk_part, ll, s));
    FC_TRY(rk45_status_launch(g, ig.rk_st, ig.rk_sum, s));
    FC_HIP(hipMemcpyAsync(ig.rk_host, ig.rk_sum, sizeof(Rk45Status), hipMemcpyDeviceToHost, s));
    // This wait is also the one fc_unet_integrate makes before its first replay: under AMD_DIRECT_DISPATCH=0 a graph submitted from this
    // thread can overtake the plain launches and copies queued just before it (see there).
    FC_HIP(hipStreamSynchronize(s));

    // (an attempt with dense output has one more launch: a different graph)
    GraphKey key = graph_key(f, per_sample ? GraphKey::Rk45PerSample : GraphKey::Rk45Coupled, cfg_strength, t_scale);
    key.dense = ev != nullptr;
    auto attempt = [&] { return enqueue_rk45_attempt(u, g, eval, cf, cfg_strength, t_scale, ev, ll, s); };
    while (ig.rk_host->unfinished > 0) {
        if (no_graph() || lk) {   // (the training-form evaluation has never been captured: the likelihood launches directly)
            FC_TRY(attempt());
        } else {   // one attempt = one graph: 6 plan runs and 10 (11 with dense output) small launches, a single chain (no parallel branches)
            hipGraphExec_t exec = nullptr;
            FC_TRY(cached_graph(u, key, s, attempt, &exec));
            FC_HIP(hipGraphLaunch(exec, s));
        }
        // the 16-byte summary behind every attempt: one small host wait per six forwards
        FC_HIP(hipMemcpyAsync(ig.rk_host, ig.rk_sum, sizeof(Rk45Status), hipMemcpyDeviceToHost, s));
        FC_HIP(hipEventRecord(ig.ev_rk, s));
        FC_HIP(hipEventSynchronize(ig.ev_rk));
    }
    std::vector<Rk45State> st(g.G);      // the controller records, once at the end
    FC_HIP(hipMemcpyAsync(st.data(), ig.rk_st, (size_t)g.G * sizeof(Rk45State), hipMemcpyDeviceToHost, s));
    FC_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < g.G; ++i) { counters[3 * i] = st[i].nfev; counters[3 * i + 1] = st[i].accepted; counters[3 * i + 2] = st[i].rejected; }
    const int failed = ig.rk_host->failed;
    if (!failed) FC_TRY(rk45_out_launch(ig.rk_y, x_dev, n, s));
    if (!failed && lk) {
        FC_HIP(hipMemcpyAsync(lk->a_out, ig.rk_a, (size_t)B * sizeof(double), hipMemcpyDeviceToDevice, s));
        FC_TRY(ode_ll_logp_launch(x_dev, lk->a_out, lk->logp_out, B, m1, s));
        if (per_probe) {      // the by-products; a_out stays the solve's own a (the mean's integral), not the mean of these
            FC_HIP(hipMemcpyAsync(lk->a_probes_out, ig.rk_ak, (size_t)K * B * sizeof(double), hipMemcpyDeviceToDevice, s));
            FC_TRY(ode_ll_mean_launch(ig.rk_ak, K, B, lk->a_out, lk->stderr_out, 1, s));
        }
    }
    FC_TRY(f.leave());
    if (!failed) return FC_OK;
    if (!per_sample) {
        if (st[0].failed == 1) return fail(FC_E_STATE, "rk45: Required step size is less than spacing between numbers.");
        return fail(FC_E_STATE, "rk45: no convergence after " + std::to_string(st[0].attempts) + " attempts (t = " +
                                    std::to_string(st[0].t) + ", h = " + std::to_string(st[0].h_abs) + ")");
    }
    std::string msg = "rk45 per sample: " + std::to_string(failed) + " of " + std::to_string(B) + " samples failed;";
    for (int b = 0; b < B; ++b) {
        if (st[b].failed == 1) msg += " sample " + std::to_string(b) + ": Required step size is less than spacing between numbers.";
        else if (st[b].failed) msg += " sample " + std::to_string(b) + ": no convergence after " + std::to_string(st[b].attempts) +
                                      " attempts (t = " + std::to_string(st[b].t) + ", h = " + std::to_string(st[b].h_abs) + ").";
    }
    return fail(FC_E_STATE, msg);
}

int fc_unet_integrate_rk45(fc_unet* u, float* x_dev, int B, int H, int W, double t0, double t1, double rtol, double atol,
                                      float t_scale, const int64_t* ids, float cfg_strength, const float* mask, int mask_is_ones,
                                      int* counters, void* stream) {
    return integrate_rk45(u, false, "fc_unet_integrate_rk45", x_dev, B, H, W, t0, t1, rtol, atol, t_scale, ids, cfg_strength, mask,
                          mask_is_ones, nullptr, 0, nullptr, counters, stream);
}

int fc_unet_integrate_rk45_per_sample(fc_unet* u, float* x_dev, int B, int H, int W, double t0, double t1, double rtol, double atol,
                                      float t_scale, const int64_t* ids, float cfg_strength, const float* mask, int mask_is_ones,
                                      int* counters, void* stream) {
    return integrate_rk45(u, true, "fc_unet_integrate_rk45_per_sample", x_dev, B, H, W, t0, t1, rtol, atol, t_scale, ids, cfg_strength,
                          mask, mask_is_ones, nullptr, 0, nullptr, counters, stream);
}

int fc_unet_integrate_rk45_dense(fc_unet* u, int per_sample, float* x_dev, int B, int H, int W, double t0, double t1, double rtol,
                                 double atol, float t_scale, const int64_t* ids, float cfg_strength, const float* mask, int mask_is_ones,
                                 const double* t_eval_host, int n_eval, float* frames_dev, int* counters, void* stream) {
    return integrate_rk45(u, per_sample != 0, "fc_unet_integrate_rk45_dense", x_dev, B, H, W, t0, t1, rtol, atol, t_scale, ids,
                          cfg_strength, mask, mask_is_ones, t_eval_host, n_eval, frames_dev, counters, stream);
}

// ---- adaptive likelihood ----------------------------------------------------------------------------------------------------------
// x from t0 back to t1 < t0 with the adaptive solve above over [x, a]: the integration error of a and z is the controller's, not a
// grid's.  The host waits on the status summary behind every attempt, as the sampler; x_inout, a_out and logp_out are written only when
// every group finished.
static int log_likelihood_rk45(const char* fn, fc_unet* u, float* x_inout, int batch, int H, int W, double t0, double t1, double rtol,
                               double atol, float t_scale, const int64_t* class_ids, const float* mask, int mask_is_ones, const float* probes,
                               int n_probes, int per_sample, double* a_out, double* logp_out, double* a_probes_out, double* stderr_out,
                               int* counters, void* stream) {
    if (!u || !x_inout || !probes || !a_out || !logp_out || !counters || batch < 1) return fail(FC_E_ARG, std::string(fn) + ": null argument");
    if (!(t1 < t0) || !(t1 >= 0.0) || !(t0 <= 1.0)) return fail(FC_E_ARG, std::string(fn) + ": needs 0 <= t1 < t0 <= 1 (data at t0 towards noise)");
    FC_TRY(check_probes(fn, n_probes, a_probes_out, stderr_out));
    FC_TRY(check_aligned16({x_inout, probes}, (std::string(fn) + ": x and the probe must be 16-byte aligned (the kernels read them as float4)").c_str()));
    const Rk45Likelihood lk{probes, a_out, logp_out, n_probes, a_probes_out, stderr_out};
    return integrate_rk45(u, per_sample != 0, fn, x_inout, batch, H, W, t0, t1, rtol, atol, t_scale, class_ids, 0.0f, mask, mask_is_ones,
                          nullptr, 0, nullptr, counters, stream, &lk);
}

int fc_unet_log_likelihood_rk45(fc_unet* u, float* x_inout, int batch, int H, int W, double t0, double t1, double rtol, double atol,
                                float t_scale, const int64_t* class_ids, const float* mask, int mask_is_ones, const float* probe,
                                int per_sample, double* a_out, double* logp_out, int* counters, void* stream) {
    return log_likelihood_rk45("fc_unet_log_likelihood_rk45", u, x_inout, batch, H, W, t0, t1, rtol, atol, t_scale, class_ids, mask,
                               mask_is_ones, probe, 1, per_sample, a_out, logp_out, nullptr, nullptr, counters, stream);
}

int fc_unet_log_likelihood_rk45_probes(fc_unet* u, float* x_inout, int batch, int H, int W, double t0, double t1, double rtol, double atol,
                                       float t_scale, const int64_t* class_ids, const float* mask, int mask_is_ones, const float* probes,
                                       int n_probes, int per_sample, double* a_out, double* logp_out, double* a_probes_out,
                                       double* stderr_out, int* counters, void* stream) {
    if (!a_probes_out || !stderr_out) return fail(FC_E_ARG, "fc_unet_log_likelihood_rk45_probes: null argument");
    return log_likelihood_rk45("fc_unet_log_likelihood_rk45_probes", u, x_inout, batch, H, W, t0, t1, rtol, atol, t_scale, class_ids, mask,
                               mask_is_ones, probes, n_probes, per_sample, a_out, logp_out, a_probes_out, stderr_out, counters, stream);
}

// The likelihood's counter-based probe field.  The key is the caller's seed moved by a constant, so that a likelihood seed does not
// replay the SDE sampler's noise of the same seed; the probe index takes the counter word the sampler's draw index has.
int fc_ode_probe_field(float* out_dev, int kind, uint64_t seed, int64_t probe_index, const int64_t* sample_ids_dev, int batch,
                       int64_t per_sample, void* stream) {
    if (!out_dev) return fail(FC_E_ARG, "fc_ode_probe_field: null argument");
    if (kind != FC_PROBE_RADEMACHER && kind != FC_PROBE_GAUSSIAN) return fail(FC_E_ARG, "fc_ode_probe_field: unknown kind");
    FC_TRY(check_aligned16({out_dev}, "fc_ode_probe_field: out must be 16-byte aligned (written as float4)"));
    if (probe_index < 0 || probe_index > 0xffffffffLL) return fail(FC_E_ARG, "fc_ode_probe_field: the probe index is a 32-bit counter word");
    if (batch < 1 || per_sample < 4 || (per_sample & 3) || (long long)batch * per_sample > 0x7fffffffLL)
        return fail(FC_E_SHAPE, "fc_ode_probe_field: elements per sample must be a positive multiple of 4, batch * per_sample < 2^31");
    const uint64_t key = seed + FC_PROBE_KEY_OFFSET;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return kind == FC_PROBE_RADEMACHER
               ? ode_rademacher_field_launch(out_dev, key, (unsigned)probe_index, sample_ids_dev, batch * (int)per_sample, (int)per_sample, s)
               : ode_probe_normal_field_launch(out_dev, key, (unsigned)probe_index, sample_ids_dev, batch * (int)per_sample, (int)per_sample, s);
}

}  // extern "C"
