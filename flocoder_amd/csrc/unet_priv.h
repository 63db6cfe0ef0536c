// The velocity U-Net object behind the fc_unet_* entry points (unet.hip: parameters, forward plan, handle lifecycle;
// unet_integrate.hip: the integrators; unet_backward.hip: backward plan of the training step).
#pragma once
#include <algorithm>
#include <map>
#include <tuple>

#include "plan.h"

namespace fc {

// What a cached graph was captured for: two calls share a graph exactly when every field agrees.
struct GraphKey {
    enum Kind { Euler, Rk4, Rk45Coupled, Rk45PerSample, Rk4Guided, Sde };
    Kind kind = Euler;
    int B = 0, mask_mode = 0;
    bool cfg_on = false, has_ids = false;
    bool pre_on = false;                                    // fixed grids: the conditioning table is in use
    bool step_close = false;                                // Euler: final_res_block's closing launch closes the step (no final_conv / init_conv launch)
    int steps = 0;                                          // fixed grids: consecutive intervals in the graph
    bool dense = false;                                     // RK45: an attempt with t_eval has one more launch
    uint32_t cfg_strength = 0, dt_euler = 0, t_scale = 0;   // the floats' bits (dt_euler: 0 for RK45)
    int sde_scheme = 0, sde_noise = 0;                      // SDE: the scheme and the noise source (0 generated, 1 supplied)
    uint32_t sde_sigma = 0;                                 // SDE: sigma's bits
    auto tie() const {
        return std::tie(kind, B, mask_mode, cfg_on, has_ids, pre_on, step_close, steps, dense, cfg_strength, dt_euler, t_scale, sde_scheme, sde_noise,
                        sde_sigma);
    }
    bool operator<(const GraphKey& o) const { return tie() < o.tie(); }
};

// Integrator state, library-owned so captured graphs never see caller pointers.  This part lives as long as the PLAN: allocated by
// fc_unet_reserve (alloc_integrator) or by the first call that needs it, always through get(); release_plan() frees and nulls the
// lot, so a lazy `if (!rk_st)` never trusts a pointer of a plan that is gone.
struct IntegratorPlanState {
    std::vector<void*> allocs;
    int* step = nullptr;                     // step counter | evaluation counter
    float *sc = nullptr, *tvec = nullptr;
    float *y = nullptr, *xs = nullptr, *k1 = nullptr, *k2 = nullptr, *k3 = nullptr, *v2 = nullptr, *mask_own = nullptr;
    int64_t* ids_own = nullptr;
    // adaptive RK45 (fc_unet_integrate_rk45 / _per_sample): state, stage derivatives, up to maxB controllers, their partial sums and the
    // status summary, allocated by the first call, so handles that never use it keep their footprint
    double *rk_y = nullptr, *rk_ynew = nullptr, *rk_part = nullptr;
    Rk45K rk_k{};
    Rk45State* rk_st = nullptr;
    Rk45Status* rk_sum = nullptr;
    // adaptive likelihood (fc_unet_log_likelihood_rk45): the divergence track a | a_new ([2][maxB]) and its K values ([7][maxB]),
    // allocated by the first call (g is ll_g below)
    // ... and with per-probe results its per-probe rows: every probe's K values ([7][ll_k][maxB]) and own integral ([ll_k][maxB])
    double *rk_a = nullptr, *rk_d = nullptr, *rk_dk = nullptr, *rk_ak = nullptr;
    // likelihood (fc_unet_log_likelihood): g = (dv/dx)^T eps of the running stage and the per-sample stage sums d1..d3 of the running
    // interval, allocated by the first call
    // With K probes per call g is [K][B][m] and the stage sums [K][B][3] (the call's B is the stride): the buffers hold ll_k probes of
    // maxB rows and grow when a call brings more (ll_reserve)
    float* ll_g = nullptr;
    double* ll_d = nullptr;
    int ll_k = 0;
    // measurement guidance (fc_unet_integrate_guided): the call's measurement and keep weights in the library's own buffers (made like
    // mask_own), {sigma_y^2, gamma} of the call, and for the exact form w and q = (dv/dx)^T w of the running stage; allocated by the
    // first call
    float *g_y = nullptr, *g_keep = nullptr, *g_sc = nullptr, *g_w = nullptr, *g_q = nullptr;
    // stochastic sampling (fc_unet_integrate_sde): the call's seed / noise pointer and its sample ids; allocated by the first call
    SdeParams* sde_prm = nullptr;
    int64_t* sde_ids = nullptr;

    template <class T> int get(T** out, size_t count, const char* tag) {
        void* p = nullptr;
        FC_TRY(dev_alloc(&p, (count ? count : 1) * sizeof(T), tag));
        allocs.push_back(p);
        *out = static_cast<T*>(p);
        return FC_OK;
    }
    // free one buffer ahead of the plan (a buffer that grows); the caller has waited for its last user
    template <class T> void drop(T** buf) {
        if (!*buf) return;
        allocs.erase(std::remove(allocs.begin(), allocs.end(), static_cast<void*>(*buf)), allocs.end());
        dev_free(*buf);
        *buf = nullptr;
    }
};
// ... and this part as long as the HANDLE (fc_unet_create makes the stream and its two events, release_handle() frees all of it).
struct IntegratorState : IntegratorPlanState {
    hipStream_t stream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    fc::Rk45Status* rk_host = nullptr;       // the pinned RK45 status summary and its event: made by the first RK45 call
    hipEvent_t ev_rk = nullptr;
    // buffers that grow on demand; captured graphs bake their addresses, so whoever moves one drops the graphs
    float* ts_dev = nullptr;                 // the time grid of the running fixed-grid call
    int ts_cap = 0;
    float* pre = nullptr;                    // conditioning of every evaluation of the running integration (CondFetch): tv | t_emb | h | c1 | ss
    size_t pre_cap = 0;                      // floats
    float* pre_ss = nullptr;                 // the [evaluation][row][S] part of `pre`
    // dense output (fc_unet_integrate_rk45_dense): the call's requested times, their count and the frames pointer, on the device like the
    // time grid, so a replayed attempt serves any request; allocated by the first such call, grows with the longest t_eval seen
    Rk45Eval* rk_ev = nullptr;
    int rk_ev_cap = 0;                       // times
    std::map<GraphKey, hipGraphExec_t> graphs;   // every cached graph: they bake the addresses of the buffers they were captured with

    void drop_graphs();
    void release_plan();
    void release_handle();
};

}  // namespace fc

struct fc_unet : fc::ParamStore {
    fc_unet_config cfg{};
    int device = 0;
    int td = 0, heads = 4;
    std::vector<int> chans;  // [dim, dim*m0, dim*m1, ...]
    int S = 0;                                    // total scale/shift width
    std::unordered_map<std::string, int> ss_off;  // resblock prefix -> column offset
    float* freqs = nullptr;

    int maxB = 0, H = 0, W = 0;
    fc::Plan plan;                           // the forward launch plan for up to maxB rows
    fc::TembArgs temb_proto;                 // weights of the conditioning chain as the plan's own launches use them
    fc::IntegratorState ig;                  // everything the integrators own (unet_integrate.hip)

    // Fused Block tails whose workgroups wait for each other (conv_dev.h) need the device to themselves.  `shared` = the caller said the
    // device is shared with other streams / processes (fc_unet_set_shared): plans are then built without such launches.  A wait that
    // times out anyway poisons its sample group with NaN and sets `dev_err`; `host_err` (pinned) receives a copy behind every forward /
    // integration, and every entry point refuses to go on once it is set (sticky until the plan is rebuilt).
    bool shared = false;
    int* dev_err = nullptr;
    volatile int* host_err = nullptr;
    bool tail_failed = false;
    hipEvent_t ev_meet = nullptr;            // end of this handle's last plan with meeting launches (process-wide guard, unet.hip)

    bool keep_all = false;   // plans keep every intermediate (q/k/v, attention output) for the backward: set by fc_unet_train_reserve

    // training (unet_backward.hip): backward launch plan over the forward arena, data-gradient weight operands
    fc::Plan bwd;
    std::vector<fc::PackJob> dgrad_packs;     // PACK_DGRAD jobs from `raw` into the plan's own operand buffers
    fc::PackTable dgrad_table;                // all of them as one launch
    uint64_t param_version = 0, dgrad_version = ~0ull;
    int64_t class_lo = 0, class_hi = 0;       // [lo, hi) of class_cond_mlp.* in the flat table
    // gradient buckets (fc_unet_backward_parts): backward plan entries [0, bwd_split_op) leave [grad_split, end) of the flat gradient vector
    // complete (final_*, mid_*, ups.*); the rest of the plan completes [0, grad_split).  bwd_split_op < 0: one bucket
    int bwd_split_op = -1;
    int64_t grad_split = 0;
    bool want_buckets = false;                // fc_unet_set_grad_buckets: build the backward plan in its two-bucket form (data-parallel trainers)

    // What the activation arena currently holds.  fc_unet_backward_ex reads the activations the LAST forward left there, so every
    // entry point that writes the arena moves `arena_serial`; `arena_train_rows` > 0 only after a forward on the keep-everything
    // (training) plan with that many rows.  A backward that does not follow such a forward fails with FC_E_STATE instead of
    // producing gradients from someone else's activations.
    uint64_t arena_serial = 0;
    int arena_train_rows = 0;
    void arena_touched(int train_rows) { ++arena_serial; arena_train_rows = train_rows; }

};

namespace fc {
// unet.hip: what every entry point that runs the plan checks, and the process-wide guard of the meeting launches
int check_ready(const fc_unet* u, int rows, int H, int W);
int check_poison(fc_unet* u);
int meet_enter(fc_unet* u, hipStream_t s);
int meet_leave(fc_unet* u, hipStream_t s);
// unet_integrate.hip: integrator state for `rows` U-Net rows of the plan just built
int alloc_integrator(fc_unet* u, int rows, int H, int W);
// unet_backward.hip: the backward plan's data-gradient chain alone (fc_unet_vjp_x, fc_unet_log_likelihood)
int vjp_check(fc_unet* u, int B, int H, int W, const char* who);
int vjp_run(fc_unet* u, const FwdCtx& c, hipStream_t s);
}  // namespace fc
