/*
 * flocoder_amd.h -- C ABI of the MI355X (gfx950) implementation of flocoder's latent-flow hot path.
 *
 * The reference (drscotthawley/flocoder @ 2025-08-08) is pure Python and has no FFI; what it has are
 * Python protocols.  Each entry point below names the reference interface it replaces (file:line in
 * the reference tree) -- INTEGRATION.md shows the ctypes stub a maintainer would add on their side.
 *
 * Conventions
 *   - every pointer marked "dev" is a DEVICE pointer owned by the caller (e.g. torch.Tensor.data_ptr());
 *     "host" pointers are plain host memory.  fp32 throughout.  Boundary tensors are NCHW contiguous,
 *     exactly the reference's layout; the library's internal activations are NHWC.
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream).  Launch functions enqueue work and
 *     return; they never allocate, free or synchronise.  Allocation happens in *_create / *_reserve only.
 *   - return value: 0 = FC_OK, negative = error; fc_last_error() gives the message (thread-local).
 *   - objects are thread-compatible: use one object per host thread.
 */
#ifndef FLOCODER_AMD_H
#define FLOCODER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FC_OK 0
#define FC_E_ARG (-1)    /* bad argument / unknown name                     -> Python ValueError   */
#define FC_E_SHAPE (-2)  /* shape the kernels do not support / not reserved -> Python ValueError   */
#define FC_E_ARCH (-3)   /* device is not gfx950                            -> Python RuntimeError */
#define FC_E_HIP (-4)    /* a HIP runtime call failed                       -> Python RuntimeError */
#define FC_E_STATE (-5)  /* weights not loaded, plan not built ...          -> Python RuntimeError */

#define FC_ABI_VERSION 1

int fc_abi_version(void);
const char* fc_last_error(void);
/* 0 if `device` is a gfx950 part, FC_E_ARCH otherwise. */
int fc_check_device(int device);

/* ------------------------------------------------------------------------------------------------
 * Velocity U-Net  (replaces flocoder/unet.py:164-377  Unet.__init__ / Unet.forward)
 * ---------------------------------------------------------------------------------------------- */
typedef struct fc_unet fc_unet;

typedef struct fc_unet_config {
    int dim;             /* Unet(dim=...)            unet.py:167 */
    int channels;        /* Unet(channels=...)       unet.py:169 */
    int n_levels;        /* len(dim_mults)           unet.py:168 */
    int dim_mults[8];
    int groups;          /* resnet_block_groups      unet.py:170 */
    int n_classes;       /* 0 = no class_cond_mlp    unet.py:172,181 */
    int mask_cond;       /* inpainting branches      unet.py:173,214-235 */
} fc_unet_config;

/* device >= 0: a gfx950 HIP device.  device < 0: description only (parameter table, no GPU touched). */
int fc_unet_create(const fc_unet_config* cfg, int device, fc_unet** out);
void fc_unet_destroy(fc_unet* u);

/* Parameter table, in the order fc_unet_load_params expects.  Names and shapes are the reference's
 * state_dict keys; `shape` receives up to 4 dims, unused = 0. */
int fc_unet_param_count(const fc_unet* u);
int fc_unet_param_info(const fc_unet* u, int i, const char** name, int64_t shape[4], int64_t* offset);
int64_t fc_unet_param_numel(const fc_unet* u);
/* Copy the flat fp32 parameter vector (all params concatenated in table order) and re-pack it into the
 * kernels' layouts.  `on_device` says whether `flat` is a device or a host pointer.
 * Replaces Unet.load_state_dict (generate_samples.py:101-106). */
int fc_unet_load_params(fc_unet* u, const float* flat, int64_t numel, int on_device, void* stream);

/* Build the launch plan and allocate the activation arena for batches up to `max_batch` of HxW latents.
 * `max_batch` counts U-Net rows: a CFG sampler of B samples needs 2B. */
int fc_unet_reserve(fc_unet* u, int max_batch, int height, int width);
/* The current reservation (0, 0, 0 before the first one).  The launch plan depends on it -- tiles are picked for max_batch rows -- so two
 * handles give bit-identical results only under equal reservations: Unet.replica() copies it (sampling.sample_many, bench.py two-in-flight). */
int fc_unet_reserved(const fc_unet* u, int* max_batch, int* height, int* width);

/* v = Unet(x, time, cond)   (unet.py:374-377).
 *   x_dev [B,C,H,W]; time_dev [B] (already multiplied by t_scale, sampling.py:63);
 *   class_ids_dev [B] int64 or NULL (cond['class_cond'] is None), an id < 0 disables the class
 *   embedding for that row; mask_dev [B,C,H,W] or NULL (cond['mask_cond']); mask_is_ones = the
 *   reference's allclose(mask,1) bypass (unet.py:301) decided by the caller; out_dev [B,C,H,W]. */
int fc_unet_forward(fc_unet* u, const float* x_dev, const float* time_dev, const int64_t* class_ids_dev,
                    const float* mask_dev, int mask_is_ones, float* out_dev, int batch, int height, int width,
                    void* stream);

/* ------------------------------------------------------------------------------------------------
 * ODE integrators  (replace flocoder/sampling.py:36-122 rk4_step / v_func_cfg / generate_latents_rk4,
 *                   and the legacy Euler loop legacy/train_sd_flowers.py:50-67)
 * ---------------------------------------------------------------------------------------------- */
#define FC_METHOD_EULER 0
#define FC_METHOD_RK4 1

/* Integrate x_dev [B,C,H,W] in place along the caller-supplied fp32 time grid.
 *   RK4  : ts_host has n_points entries (= warp_time(linspace(...)), sampling.py:102-111); the loop runs
 *          n_points-1 intervals with stages at t, t+dt/2, t+dt/2, t+dt  (sampling.py:43-48,116-117).
 *   Euler: ts_host has n_points = N entries t_i = i/N*(1-eps)+eps; x += v*dt with dt_euler = 1/N
 *          (train_sd_flowers.py:58-64).
 *   t_scale multiplies every time value before it reaches the U-Net (999, sampling.py:57).
 *   class_ids_dev/mask_dev as in fc_unet_forward.  cfg_strength != 0 with class ids present runs the
 *   classifier-free-guidance pair as one 2B-row pass (sampling.py:69-74).
 * A run of consecutive integration steps (as many as fit ~6000 graph nodes: all 64 of the Euler sampler) is captured in a hipGraph
 * the first time a (method, B, H, W, cfg, mask, run length) variant is seen and replayed from then on; step counter, time grid and
 * conditioning table live in device memory, so replays take any grid.  On return the trajectory is queued on `stream`, not finished:
 * fc_unet_check(u, stream, 1) waits for it and reports a timed-out cross-workgroup wait (see fc_unet_set_shared). */
int fc_unet_integrate(fc_unet* u, int method, float* x_dev, int batch, int height, int width,
                      const float* ts_host, int n_points, float dt_euler, float t_scale,
                      const int64_t* class_ids_dev, float cfg_strength, const float* mask_dev, int mask_is_ones,
                      void* stream);

/* Adaptive RK45: scipy.integrate.solve_ivp(f, (t0, t1), y0, method="RK45", rtol, atol) as the legacy evaluation sampler calls it
 * (legacy/train_sd_flowers.py:78-107), with f(t, y) = U-Net(float32(y), float32(t) * t_scale) [CFG-blended as fc_unet_integrate].
 * scipy 1.15 semantics (_ivp/rk.py, _ivp/common.py): Dormand-Prince 5(4) with FSAL, select_initial_step, RMS error norm over ALL
 * batch*C*H*W unknowns -- ONE step size for the whole batch, so a sample's trajectory depends on the rest of its batch, as upstream.
 * y, y_new, stage sums and the error are fp64; the forwards take and return fp32.  x_dev [B,C,H,W] is replaced by float32(y(t1)).
 * counters[3] (host) = { nfev (scipy's solution.nfev; a CFG pair counts once), accepted steps, rejected attempts }.
 * atol < 0 -> FC_E_ARG; rtol below 100 eps is raised to 100 eps.  A step below the spacing of t ("Required step size is less than
 * spacing between numbers.") or an internal cap on attempts -> FC_E_STATE, x_dev untouched.
 * One attempt (6 forwards + 10 small launches) is a captured hipGraph per (B, cfg, mask, class ids) variant; the controller runs on
 * the device and the host reads a 16-byte status summary behind each replay.  Unlike fc_unet_integrate this call is SYNCHRONOUS with respect to
 * the library stream (it must see when the solve ends): on return the result is queued on `stream` behind the solve.  The extra
 * state (fp64 y / y_new, K0..K6) is allocated by the first call, not by fc_unet_reserve. */
int fc_unet_integrate_rk45(fc_unet* u, float* x_dev, int batch, int height, int width, double t0, double t1, double rtol, double atol,
                           float t_scale, const int64_t* class_ids_dev, float cfg_strength, const float* mask_dev, int mask_is_ones,
                           int* counters, void* stream);

/* Adaptive RK45 with one solve per sample: every sample b is its OWN scipy.integrate.solve_ivp(f_b, (t0, t1), y0_b, method="RK45",
 * rtol, atol) problem over its C*H*W unknowns, f_b = the U-Net forward on that sample alone (its class id, its mask row, CFG as
 * fc_unet_integrate_rk45).  Each sample has its own select_initial_step, RMS error norm, step size, accept / reject decisions and
 * counters, so its result depends only on its own source, class id and mask -- not on the batch size or on its batchmates -- and a
 * batch may be split across calls or ranks.  The arithmetic is fc_unet_integrate_rk45's (fp64 state, stage sums and norms, fp32
 * forwards); the norms' partial sums are partitioned by C*H*W alone and reduced in a fixed order.  A sample that has finished stays
 * in the batch with h = 0 (its rows are still evaluated; its state and counters are frozen), so the call makes max_b nfev_b batch
 * forwards.  counters[3 * batch] (host) = { nfev, accepted, rejected } per sample.  atol < 0 -> FC_E_ARG; rtol below 100 eps is
 * raised to 100 eps; t0 == t1 -> nfev 1 each, x_dev untouched.  If any sample fails (step below the spacing of its t, or the attempt
 * cap) -> FC_E_STATE with the failing sample indices and reasons in fc_last_error(), x_dev untouched.  One attempt (6 forwards + 10
 * small launches) is a captured hipGraph per (B, cfg, mask, class ids) variant; the host reads a 16-byte summary (samples still
 * stepping, samples failed) behind each replay, so the call is SYNCHRONOUS like its sibling.  Its extra state is allocated by the
 * first call, sized by the reserved batch. */
int fc_unet_integrate_rk45_per_sample(fc_unet* u, float* x_dev, int batch, int height, int width, double t0, double t1, double rtol,
                                      double atol, float t_scale, const int64_t* class_ids_dev, float cfg_strength, const float* mask_dev,
                                      int mask_is_ones, int* counters /* host, [3*batch] */, void* stream);

/* Either adaptive RK45 solve with the trajectory at requested times: solve_ivp's `t_eval`.  per_sample == 0 is
 * fc_unet_integrate_rk45, otherwise fc_unet_integrate_rk45_per_sample; every argument they share means what it means there
 * (counters[3] or counters[3 * batch]).  The step sequence is untouched: x_dev and the counters get the bits of the call without
 * t_eval.  After every accepted step of a controller (the batch's one, or each sample's own) every not-yet-served t_eval[j] with
 * dir * (t_eval[j] - t) <= 0 is evaluated from that step's quartic interpolant (scipy's RkDenseOutput: y_old + h Q p, Q = K^T P over the
 * seven stage derivatives the step already holds; fp64, no extra evaluation) and written as frame j of that controller's rows:
 * frames_dev [n_eval, batch, C, H, W] fp32, caller-owned, 16-byte aligned, written on the library's stream and ordered before `stream`
 * continues, like x_dev.  A time equal to t0 yields the source; the frame at t1 is the interpolant there, equal to x_dev to rounding.
 * t_eval_host: n_eval fp64 times on the host (read before the call returns), inside [t0, t1] and strictly monotonic in the direction
 * of integration, else FC_E_ARG with scipy's wording ("Values in `t_eval` are not within `t_span`." / "Values in `t_eval` are not
 * properly sorted.").  n_eval == 0 is the plain call.  t0 == t1: every frame is the source.  On FC_E_STATE (a failed solve) the
 * frames hold no promise.  The times, their count and frames_dev live in device memory of the handle, so the captured attempt (one
 * more small launch than the plain one, its own graph) is replayed for any request. */
int fc_unet_integrate_rk45_dense(fc_unet* u, int per_sample, float* x_dev, int batch, int height, int width, double t0, double t1,
                                 double rtol, double atol, float t_scale, const int64_t* class_ids_dev, float cfg_strength,
                                 const float* mask_dev, int mask_is_ones, const double* t_eval_host, int n_eval, float* frames_dev,
                                 int* counters, void* stream);

/* Kept for compatibility: the reserved batch always runs as ONE chain of rows on one stream, so this returns 1 and sets
 * *rows_per_chain to the reserved batch (0 before fc_unet_reserve). */
int fc_unet_chains(const fc_unet* u, int* rows_per_chain);
/* Number of kernel launches in one U-Net forward of the current plan. */
int fc_unet_plan_launches(const fc_unet* u);
/* Fused Block tails meet the workgroups of a sample at a device-side counter (bounded wait).  *count = launches whose wait ever
 * timed out since the plan was built -- must be 0; anything else means the residency assumption broke and results are invalid.
 * Synchronises. */
int fc_unet_fused_tail_errors(const fc_unet* u, int* count);
/* Device sharing.  The default ("exclusive") plan closes most Blocks inside their second convolution by letting the workgroups of a
 * sample exchange GroupNorm partials inside the launch; such a launch is only correct while its whole grid is resident, i.e. while
 * nothing else competes for the CUs.  Within one process the library orders these plans against each other across streams by itself.
 * A caller that runs the handle beside other GPU work it does not order against (a second replica meant to overlap, collectives of a
 * training job, another process on the same GPU) declares that with shared = 1: plans are then built without cross-workgroup waits
 * (same results to fp32 rounding -- the GroupNorm partials are combined in another order --, one more launch per Block).  Changing the mode drops the current plan; the next reserve rebuilds it.
 * No counterpart in the reference (PyTorch kernels never wait for each other). */
int fc_unet_set_shared(fc_unet* u, int shared);
/* Launches of the current plan whose workgroups wait for each other (0 for a shared-mode or training plan). */
int fc_unet_meeting_launches(const fc_unet* u);
/* Has a wait of such a launch ever timed out?  A timed-out wait turns its samples into NaN (never finite garbage) and makes every later
 * call on the handle -- this one included -- return FC_E_STATE until the plan is rebuilt.  With `synchronize` != 0 the call first waits
 * for `stream` (the stream the last forward / integration was given), so that its answer covers that work. */
int fc_unet_check(fc_unet* u, void* stream, int synchronize);
/* Test hook: makes the next run of the plan's first meeting launch time out. */
int fc_debug_unet_break_meeting(fc_unet* u);
int fc_debug_unet_break_meeting_kind(fc_unet* u, int kind);   /* kind: 0 a convolution's Block tail, 1 the linear attention's fused close */
/* Experiment switch: plans built after the call use (1) / do not use (0) the launches whose workgroups meet (cross-workgroup Block
 * tails, the linear attention's fused close; tile-local Block tails stay); < 0 restores the default (on). */
int fc_debug_set_fused_tail(int on);
/* FLOPs per sample and evaluation as the REFERENCE computes the network (2 x MACs of every module, unet.py:289-372; SURVEY 8(d): 1.0008e9 at
 * dim 32) -- the unit of every end-to-end TFLOP/s figure.  Inference plans execute less where nn.Upsample + conv3x3 is folded into four 2x2
 * kernels (9 -> 4 taps per output pixel): fc_unet_op_info reports what each launch executes. */
double fc_unet_flops_per_sample(const fc_unet* u);
/* Launch i of the plan: kernel family, the reference module it implements, the FLOPs per sample it executes. */
int fc_unet_op_info(const fc_unet* u, int i, const char** kernel, const char** module, double* flops_per_sample);
/* Algorithmic HBM bytes of launch i (convolution launches; 0 for the others): per sample = every input / output / residual element
 * once, per launch = the weights once -- the figure bench.py's roofline.traffic is read against. */
int fc_unet_op_bytes(const fc_unet* u, int i, double* bytes_per_sample, double* bytes_per_launch);
/* Measurement hook for bench.py: average device milliseconds of every launch of the plan at `batch` rows, each
 * timed alone with HIP events on `stream` over `repeats` back-to-back launches.  Synchronises. */
int fc_unet_profile_ops(fc_unet* u, int batch, int repeats, float* ms_out, int n_out, void* stream);

/* The sinusoidal frequency table exp(-k ln(1e4)/(dim/2-1)) (unet.py:26-27).  The library builds it in double
 * precision; a host that wants the exact fp32 values its own framework produces may override it. */
int fc_unet_set_time_freqs(fc_unet* u, const float* freqs_host, int n);

/* Log-likelihood of x_inout_dev [B,C,H,W] under the flow, with a Hutchinson estimate of the divergence: the classic RK4 step along
 * ts_host (n_points >= 2 entries; the caller passes the sampler's grid reversed, t = 1 -> 0), every stage a training-mode forward plus
 * fc_unet_vjp_x's chain with probe_dev [B,C,H,W] as output cotangent:
 *     x <- x + (dt/6)(v1 + 2 v2 + 2 v3 + v4)                         fp32, the arithmetic of fc_unet_integrate(FC_METHOD_RK4)
 *     a[b] <- a[b] + (double(dt)/6)(d1 + 2 d2 + 2 d3 + d4)[b]        d_j[b] = sum_i probe[b,i] ((dv_j/dx_j)^T probe)[b,i], fp64, fixed order
 * On return (queued on `stream`, asynchronous like fc_unet_integrate) x_inout_dev is the state at ts[n_points-1] (the noise z),
 * a_out_dev [B] the integrated divergence and logp_out_dev [B] = -|z_b|^2/2 - (CHW/2) ln 2pi + a[b].  No classifier-free guidance (the
 * guided field is not the flow of a density the model defines).  probe_dev must be 16-byte aligned.  Needs fc_unet_train_reserve for this shape; writes the activation
 * arena (fc_unet_arena_serial moves; a backward must re-run its forward). */
int fc_unet_log_likelihood(fc_unet* u, float* x_inout_dev, int batch, int height, int width, const float* ts_host, int n_points,
                           float t_scale, const int64_t* class_ids_dev, const float* mask_dev, int mask_is_ones, const float* probe_dev,
                           double* a_out_dev, double* logp_out_dev, void* stream);

/* fc_unet_log_likelihood with error control: scipy's solve_ivp(method="RK45") -- the controller of fc_unet_integrate_rk45 (per_sample
 * == 0: one controller group over the batch) / fc_unet_integrate_rk45_per_sample (per_sample != 0: one per sample) -- from t0 back to
 * t1 (0 <= t1 < t0 <= 1, else FC_E_ARG) on the concatenated state of a group, y = [x (m unknowns), a (one per row)], dy/dt = [v, d] with
 * d[b] = sum_i probe[b,i] ((dv/dx)^T probe)[b,i] and a = 0 at t0: select_initial_step and the RMS error norm run over m + rows unknowns,
 * the a-component's scale is atol + rtol max(|a|, |a_new|).  x as in fc_unet_integrate_rk45 (fp64 state, fp32 forwards as K); a, its
 * seven K values and its terms of the norms fp64, added after the group's x partial sums, one term per row in row order (two calls
 * give equal bits).  Every evaluation is a training-form forward plus fc_unet_vjp_x's chain with probe_dev as cotangent, launched
 * directly; needs fc_unet_train_reserve for this shape (else FC_E_STATE); no classifier-free guidance.  Synchronous like
 * fc_unet_integrate_rk45; counters: [3] (per_sample == 0) or [3 * batch] host ints, nfev / accepted / rejected per group.  On success
 * x_inout_dev holds z = x(t1), a_out_dev [B] the integrated divergence, logp_out_dev [B] = -|z_b|^2/2 - (CHW/2) ln 2pi + a[b]; on
 * FC_E_STATE (scipy's failure messages, per sample naming the samples) none of the three is written.  x_inout_dev and probe_dev must
 * be 16-byte aligned.  Writes the activation arena like fc_unet_log_likelihood. */
int fc_unet_log_likelihood_rk45(fc_unet* u, float* x_inout_dev, int batch, int height, int width, double t0, double t1, double rtol,
                                double atol, float t_scale, const int64_t* class_ids_dev, const float* mask_dev, int mask_is_ones,
                                const float* probe_dev, int per_sample, double* a_out_dev, double* logp_out_dev, int* counters,
                                void* stream);

/* Both likelihoods with K = n_probes Hutchinson probes in one solve.  probes_dev [K][B][C*H*W] fp32, 16-byte aligned;
 * 1 <= K <= FC_LL_MAX_PROBES (else FC_E_ARG, the message names the cap): the library's input-gradient buffer grows to K * maxB * C*H*W
 * floats on first use and is released with the plan.  The trajectory does not depend on the probe, so every evaluation is ONE
 * training-form forward followed by K data-gradient chains, probe k as the cotangent of chain k, and
 *     d_{s,k}[b] = sum_i probe_k[b,i] ((dv/dx)^T probe_k)[b,i]             the single-probe reduction, per probe
 * RK4 grid: every probe has its own accumulator, a_k <- a_k + (double(dt)/6)(((d1 + 2 d2) + 2 d3) + d4) on its own d's, so
 * a_probes_out_dev[k] has the bits of fc_unet_log_likelihood's a_out_dev with probe k; a_out_dev = (a_1 + ... + a_K) / K summed in probe
 * order with one division.  RK45: the augmented state stays [x, a] with da/dt = (d_{s,1} + ... + d_{s,K}) / K (same order, one
 * division), which is what every norm reads, n = m + rows as before; a_out_dev is that a.  The per-probe integrals are by-products
 * outside the norm: the controller thread that commits an accepted step also sets a_k <- a_k + h sum_s B_s d_{s,k}, formed as a_new is.
 * Both: logp_out_dev from a_out_dev as before; a_probes_out_dev [K][B] fp64; stderr_out_dev [B] fp64 =
 * sqrt(sum_k (a_k - a)^2 / (K (K - 1))), NaN for K = 1.  K = 1 runs the arithmetic of the single-probe entry points, which are this
 * routine with K = 1 and no per-probe outputs.  Everything else (arguments, alignment, asynchrony / synchrony, counters, failure: nothing
 * written) as the entry point each extends. */
#define FC_LL_MAX_PROBES 64
int fc_unet_log_likelihood_probes(fc_unet* u, float* x_inout_dev, int batch, int height, int width, const float* ts_host, int n_points,
                                  float t_scale, const int64_t* class_ids_dev, const float* mask_dev, int mask_is_ones,
                                  const float* probes_dev, int n_probes, double* a_out_dev, double* logp_out_dev,
                                  double* a_probes_out_dev, double* stderr_out_dev, void* stream);
int fc_unet_log_likelihood_rk45_probes(fc_unet* u, float* x_inout_dev, int batch, int height, int width, double t0, double t1, double rtol,
                                       double atol, float t_scale, const int64_t* class_ids_dev, const float* mask_dev, int mask_is_ones,
                                       const float* probes_dev, int n_probes, int per_sample, double* a_out_dev, double* logp_out_dev,
                                       double* a_probes_out_dev, double* stderr_out_dev, int* counters, void* stream);
/* The likelihood's counter-based probe field: out_dev [batch, per_sample] (fp32, 16-byte aligned, per_sample a multiple of 4) for probe
 * index probe_index (a 32-bit counter word) and the given sample ids (NULL: 0 .. batch-1).  Philox4x32-10 with key = seed +
 * FC_PROBE_KEY_OFFSET (mod 2^64; so a likelihood seed does not replay fc_unet_integrate_sde's noise of the same seed) and counter
 * (float4 group inside the sample, probe_index, sample id): a value depends on (seed, probe index, sample id, position) and on nothing
 * else.  FC_PROBE_RADEMACHER: +1 where the top bit of the element's Philox word is clear, -1 where it is set.  FC_PROBE_GAUSSIAN:
 * fc_ode_normal_field's uniforms and Box-Muller transform under that key, evaluated in fp64 and rounded once to fp32 (a probe field is
 * drawn once per call, so it can afford the host form's arithmetic and have its bits), |value| <= sqrt(48 ln 2) = 5.77. */
#define FC_PROBE_RADEMACHER 0
#define FC_PROBE_GAUSSIAN 1
#define FC_PROBE_KEY_OFFSET 0x50524F4245464C44ULL /* "PROBEFLD" */
int fc_ode_probe_field(float* out_dev, int kind, uint64_t seed, int64_t probe_index, const int64_t* sample_ids_dev, int batch,
                       int64_t per_sample, void* stream);

/* Measurement-guided RK4 sampling: the training-free inverse-problem method of the reference (flocoder/inpainting.py:92-130 algorithm3)
 * for a diagonal measurement operator on the conditional-OT path.  fc_unet_integrate(FC_METHOD_RK4) along ts_host (n_points >= 2, every
 * point > 0) in which every stage velocity v -- after classifier-free guidance -- produced at stage state x and stage time t becomes
 *     x1 = x + (1-t) v     w = keep (y_meas - keep x1) / (r2 keep^2 + sigma_y^2)  (0 where that is 0/0)     r2 = (1-t)^2 / (t^2 + (1-t)^2)
 *     v <- v + gamma ((1-t)/t) g        g = w (FC_JACOBIAN_IDENTITY, what the reference computes)
 *                                       g = w + (1-t) (dv/dx)^T w (FC_JACOBIAN_EXACT: d x1 / d x = I + (1-t) dv/dx)
 * y_meas_dev, keep_dev [B,C,H,W] (keep weights in [0,1]; for inpainting y_meas = keep * known latents) are copied into the library's
 * own buffers; they and x_dev must be 16-byte aligned.  1-t, r2 and gamma (1-t)/t are formed in fp64 from the fp32 stage time and
 * rounded once; the elementwise part is single-rounded fp32 in the order written above.  A zero correction term (gamma = 0, keep = 0,
 * t = 1) leaves the bits of fc_unet_integrate.
 * Identity: captured and replayed like fc_unet_integrate (sigma_y and gamma live in device memory, so one graph serves all values);
 * class ids, guidance and mask conditioning as there.  Exact: every evaluation is a training-form forward plus fc_unet_vjp_x's chain with
 * w as cotangent, direct launches as fc_unet_log_likelihood; needs fc_unet_train_reserve (else FC_E_STATE) and takes no classifier-free
 * guidance (FC_E_ARG).  A grid point <= 0, sigma_y < 0 or a misaligned pointer -> FC_E_ARG.  Asynchronous like fc_unet_integrate. */
#define FC_JACOBIAN_IDENTITY 0
#define FC_JACOBIAN_EXACT 1
int fc_unet_integrate_guided(fc_unet* u, float* x_dev, int batch, int height, int width, const float* ts_host, int n_points, float t_scale,
                             const int64_t* class_ids_dev, float cfg_strength, const float* mask_dev, int mask_is_ones,
                             const float* y_meas_dev, const float* keep_dev, float sigma_y, float gamma, int jacobian, void* stream);
/* The identity-form correction of one evaluation on caller tensors of n elements (a multiple of 4, 16-byte aligned):
 * out = v + gamma ((1-t)/t) w with the arithmetic of fc_unet_integrate_guided; t > 0, sigma_y >= 0.  out_dev may be v_dev. */
int fc_ode_guided_correct(const float* v_dev, const float* x_dev, const float* y_dev, const float* a_dev, int64_t n, float t, float sigma_y,
                          float gamma, float* out_dev, void* stream);

/* Stochastic sampling: the SDE that shares the marginals of the probability-flow ODE on the linear path x_t = (1-t) x0 + t x1 with
 * diffusion sigma^2 (1-t),
 *     dx = b(x,t) dt + sigma sqrt(1-t) dW        b(x,t) = (1 + sigma^2 t / 2) v(x,t) - (sigma^2 / 2) x
 * (v after classifier-free guidance), along ts_host (n_points >= 2, non-decreasing, within [0, 1]).  Interval i with h = t_{i+1} - t_i,
 * a = sigma sqrt(h (1 - (t_i + t_{i+1})/2)) and xi ~ N(0, I):
 *     FC_SDE_EULER_MARUYAMA   x+ = x + h b(x,t_i) + a xi                                             (1 evaluation)
 *     FC_SDE_HEUN             xp = x + h b(x,t_i) + a xi;  x+ = x + (h/2)(b(x,t_i) + b(xp,t_{i+1})) + a xi   (2 evaluations, one xi)
 * sigma = 0 is deterministic Euler / Heun on the grid.  xi is slice i of noise_dev (fp32 [n_points-1, B, C, H, W], 16-byte aligned, read
 * while the call runs) or, with noise_dev NULL, the library's counter-based normal field: Philox4x32-10, key = seed, counter =
 * (float4 group inside the sample, i, sample id) with sample_ids_dev [B] (int64; NULL: 0 .. B-1) -- a sample's noise depends on its id,
 * not on its row or the batch size.  h, a and the two drift coefficients are formed in fp64 from the fp32 grid and sigma and rounded
 * once; the elementwise part is single-rounded fp32.  Captured and replayed like fc_unet_integrate (seed, ids and the noise pointer live
 * in device memory: one graph serves all of them); class ids, guidance, mask conditioning and asynchrony as there. */
#define FC_SDE_EULER_MARUYAMA 0
#define FC_SDE_HEUN 1
int fc_unet_integrate_sde(fc_unet* u, int scheme, float* x_dev, int batch, int height, int width, const float* ts_host, int n_points,
                          float t_scale, const int64_t* class_ids_dev, float cfg_strength, const float* mask_dev, int mask_is_ones,
                          float sigma, uint64_t seed, const int64_t* sample_ids_dev, const float* noise_dev, void* stream);
/* out_dev [batch, per_sample] (fp32, 16-byte aligned, per_sample a multiple of 4) = the normal field of fc_unet_integrate_sde for draw
 * (interval) index draw_index and the given sample ids (NULL: 0 .. batch-1).  |value| <= sqrt(48 ln 2) = 5.77. */
int fc_ode_normal_field(float* out_dev, uint64_t seed, int64_t draw_index, const int64_t* sample_ids_dev, int batch, int64_t per_sample,
                        void* stream);

/* Inpainting masks (replace flocoder/inpainting.py:277-351 generate_mask, restated counter-based): masks_out_dev [batch, 1, height, width]
 * fp32 0/1 and types_out_dev [batch] int32 (the FC_MASK_* code chosen) for the given sample ids (int64; NULL: 0 .. batch-1; negative and
 * > 2^32 are legal).  A mask depends on (seed, sample id, height, width, the type probabilities or the forced type) and on nothing else --
 * not on its row, the batch or the stream.  Philox4x32-10 with key = seed + FC_MASK_KEY_OFFSET (mod 2^64) and counter (j, region, sample
 * id); csrc/masks.hip has the regions, flocoder_amd/noise.py mask_field is the host form and agrees in every bit (all draws and the brush
 * walk are integer arithmetic; the walk's sine / cosine come from the committed table csrc/mask_trig.h).
 * Type: forced_type >= 0 gives every sample that type (the choices are not read); otherwise word 0 of the sample's first block against the
 * cumulative probs_host [n_choices] (fp64, each in [0, 1], sum 1 to 1e-8; 1 <= n_choices <= 16) of choice_types_host [n_choices]: the
 * thresholds are floor(cum_k 2^32) with cum summed left to right in fp64, the last one 2^32.  Both arrays are host memory, read during the
 * call.  16 <= height, width <= 1024, else FC_E_SHAPE.  One launch on `stream`, one workgroup per sample; no allocation, no host wait. */
#define FC_MASK_TOTAL 0
#define FC_MASK_BRUSH 1
#define FC_MASK_RECTANGLES 2
#define FC_MASK_NOISE 3
#define FC_MASK_NOTHING 4
#define FC_MASK_MIN_SIZE 16
#define FC_MASK_MAX_SIZE 1024
#define FC_MASK_KEY_OFFSET 0x4D41534B464C4431ULL /* "MASKFLD1" */
int fc_inpaint_masks(float* masks_out_dev, int* types_out_dev, uint64_t seed, const int64_t* sample_ids_dev, int batch, int height, int width,
                     const int* choice_types_host, const double* probs_host, int n_choices, int forced_type, void* stream);

/* Confusion counts of a piano roll against its target (replace flocoder/metrics.py:362-455 calc_note_metrics up to the ratios, which
 * the caller forms from these exact totals).  pred_dev [batch, pred_channels, height, width] and target_dev [batch, target_channels,
 * height, width] fp32, channels 1 or 3 each on its own: 3 is taken as it is, 1 goes through g2rgb (red = gf >= 0.75, green =
 * |gf - 0.5| < 0.25, blue = 0; keep_gray != 0: gf > 0.5 on all three).  Per pixel, for channel 0 (onset) and 1 (sustain), in fp32 and
 * upstream's operation order:  t = ((target - lo) / range) > threshold,  p = ((clamp(pred, lo, hi) - lo) / range) > threshold  with
 * torch's clamp (NaN stays NaN and compares false).  lo = minval and hi = maxval rounded to fp32, or with derive_min / derive_max != 0 the
 * min / max of the WHOLE converted target (NaN if it holds one, as torch), found by a first launch; range = float(maxval - minval) when
 * both are given, hi - lo in fp32 otherwise.  An all-black target makes range 0: every comparison is false, every pixel a true negative.
 * region_dev: NULL or [batch, 1, height, width] fp32; a pixel with region <= 0.5 is counted nowhere and is 0 in every image.
 * ws_dev: 16 bytes of caller-owned scratch.  counts_out_dev [2][batch][4] int64 (onset | sustain; tp, tn, fp, fn per sample) is
 * zeroed and written by the call.  masks_out_dev [2][4][batch][height*width] fp32 (tp, tn, fp, fn as 0 / 1) and overlay_out_dev
 * [2][batch][3][height*width] (target bit, pred bit, 0) are both given or both NULL.  16-byte loads and stores when height*width is a
 * multiple of 4 and every tensor pointer is 16-byte aligned, otherwise one pixel per lane: a misaligned base is handled.  Channels other
 * than 1 / 3 -> FC_E_SHAPE.  Two memsets and one or two launches on `stream`; no allocation, no host wait. */
int fc_note_confusion(const float* pred_dev, int pred_channels, const float* target_dev, int target_channels, const float* region_dev, int batch,
                      int height, int width, float threshold, double minval, int derive_min, double maxval, int derive_max, int keep_gray,
                      void* ws_dev, int64_t* counts_out_dev, float* masks_out_dev, float* overlay_out_dev, void* stream);

/* Codebook usage (replace the counting of flocoder/codebook_analysis.py:28-44): indices_dev [n][levels] int64, the layout
 * fc_rvq_quantize writes; counts_inout_dev [levels][codebook_size] int64 is ADDED to, so a caller accumulates over calls;
 * keys_out_dev NULL or [n] int64, key = sum_l index_l codebook_size^l (FC_E_SHAPE when codebook_size^levels overflows int64).
 * A row with an index outside [0, codebook_size) is counted at no level, gets key -1 and adds one to *bad_rows_inout_dev (device int64,
 * required): the caller reads that word when it next reads the counts.  levels * codebook_size <= FC_HIST_LDS_BINS: 32-bit bins in LDS
 * per workgroup, one 64-bit global atomic per non-zero bin at the end; above: one 64-bit global atomic per index.  One launch on
 * `stream` (none for n == 0); no allocation, no host wait. */
#define FC_HIST_LDS_BINS 8192
int fc_index_histogram(const int64_t* indices_dev, int64_t n, int levels, int codebook_size, int64_t* counts_inout_dev, int64_t* keys_out_dev,
                       int64_t* bad_rows_inout_dev, void* stream);

/* Pre-encoding augmentation from a resident image pool (replace flocoder/data.py:49-111 image_transforms / midi_transforms; the
 * definitions are flocoder_amd/noise.py augment_image_field / augment_midi_field).  pool_dev: one uint8 buffer of HWC images;
 * table_dev [n_sources][4] int64 (16-byte aligned) = (byte offset, H, W, C) per source, C = 1 or 3, H, W <= FC_AUG_MAX_SIDE (the caller vouches that
 * offset + H W C lies inside the pool; the kernels check every coordinate against H and W).  The random draws are made on the host
 * (noise.py, Philox key = seed + FC_AUG_KEY_OFFSET) and reach the device as an integer table per sample, so a source pixel is the same
 * integer decision on both sides; a sample whose source index lies outside [0, n_sources) reads nothing and comes out as `fill`
 * (images) or zero (MIDI).  One launch on `stream` each; no allocation, no host wait.
 *
 * fc_augment_images: out_dev [batch, 3, size, size] fp32; sample_table_dev [batch][FC_AUG_IMAGE_WORDS] int32 =
 *   (source, a0, a1, a2, a3, a4, a5, crop left, crop top, crop side, box x0, box y0, box w, box h, flip, 0):
 *   the rotated image R (the source's size) is R[Y][X] = source[(a3 X + a4 Y + a5) >> 16][(a0 X + a1 Y + a2) >> 16] or `fill` outside
 *   (Q16 coefficients, 64-bit products); the centre crop is R[top .. top + side)[left .. left + side); the box lies in the crop's
 *   coordinates and is resized to size x size with a tent of half-width max(1, box / size) per axis, taps clamped to the crop, weights
 *   integer numerators over their integer sum; flip != 0 mirrors the columns; value = (v / 255 - mean[c]) / std[c].  mean, std, fill:
 *   three host floats each, fill in output units.  16 <= size <= 1024, std finite and > 0, else FC_E_SHAPE / FC_E_ARG.
 *   A workgroup per 16 x 16 output tile: the tile's window of R goes to LDS as bytes when it has at most FC_AUG_LDS_PIXELS pixels and is
 *   read through L2 otherwise.
 * fc_augment_midi: out_dev [batch, out_channels, size, size] fp32; sample_table_dev [batch][FC_AUG_MIDI_WORDS] int32 =
 *   (source, shift x, shift y, crop left, crop top, 0, 0, 0): u_c[y][x] = source[y + top - shift y][x + left - shift x][c] / 255 in fp32,
 *   0 outside (a translation with zero fill); gray != 0: g = min(max((u_0 + u_1) + u_2, 0), 1) on every output channel, otherwise
 *   output channel k is source channel k (channel 0 of a one-channel source); threshold > 0: 1 where the value >= threshold else 0.
 *   out_channels 1 or 3. */
#define FC_AUG_KEY_OFFSET 0x415547464C443031ULL /* "AUGFLD01" */
#define FC_AUG_MIN_SIZE 16
#define FC_AUG_MAX_SIZE 1024
#define FC_AUG_MAX_SIDE 8192
#define FC_AUG_IMAGE_WORDS 16
#define FC_AUG_MIDI_WORDS 8
#define FC_AUG_LDS_PIXELS 6144
int fc_augment_images(float* out_dev, const uint8_t* pool_dev, const int64_t* table_dev, int n_sources, const int* sample_table_dev, int batch,
                      int size, const float* mean_host, const float* std_host, const float* fill_host, void* stream);
int fc_augment_midi(float* out_dev, const uint8_t* pool_dev, const int64_t* table_dev, int n_sources, const int* sample_table_dev, int batch,
                    int size, int out_channels, int gray, float threshold, void* stream);

/* ---- debug / test hooks: not part of the drop-in surface --------------------------------------- */
/* After an exact-form fc_unet_integrate_guided call: device pointers to the last stage's input state [B,C,H,W], its scaled time rows [B],
 * its w and q = (dv/dx)^T w, while the plan that ran it stands. */
int fc_debug_unet_guided_buffers(const fc_unet* u, const float** stage_x, const float** stage_time, const float** w, const float** q);
/* out_dev[b] (double) = sum_i probe_dev[b,i] g_dev[b,i] over per_sample elements: the likelihood stage kernels' reduction alone. */
int fc_debug_probe_dot(const float* probe_dev, const float* g_dev, double* out_dev, int batch, int64_t per_sample, void* stream);
/* Device pointer + NHWC extent of an internal activation of the current plan, by reference module name
 * ("downs.0.0", "downs.0.2", "mid_attn", "ups.3.3", ...). */
int fc_unet_debug_tensor(const fc_unet* u, const char* name, const float** ptr, int* channels, int* height, int* width);
int fc_debug_copy(void* dst_dev, const void* src_dev, int64_t bytes, void* stream);
/* Memory diagnostics (csrc/devmem.hip): with the switch on (or FLOCODER_AMD_POISON=1 in the environment) every long-lived buffer the
 * library allocates FROM THEN ON -- arenas, statistics, integrator state, parameter stores, job tables -- is filled with 0xFFFFFFFF words
 * (NaN as fp32) and fenced by 64 KiB of the same pattern on both sides: a value read before it was written, or read past a buffer's end,
 * poisons the result instead of depending on what the memory held before; fc_debug_poison_check counts the buffers whose fences were
 * WRITTEN (fc_last_error names them) and synchronises the device. */
int fc_debug_set_poison(int on);
int fc_debug_poison_check(int* corrupted, int* live);
/* Diagnostics: subsequent pipelined-conv launches write shader-clock phase stamps to buf_dev
 * ([block][wave][16] uint64); NULL switches them off again. */
int fc_debug_set_conv_stamps(void* buf_dev);
/* Diagnostics: fc_debug_conv_routes(1) starts an empty record of the instantiation every pipelined-conv launch goes to (one line of its thirteen
 * template arguments per launch, in launch order; the twelfth is the geometry key of a Block-closing flavour, the thirteenth that of a
 * conv1 flavour), 0 stops; fc_debug_conv_routes_read copies it (NUL-terminated, truncated to cap) and
 * returns its full length. */
int fc_debug_conv_routes(int on);
int fc_debug_conv_routes_read(char* buf, int cap);
/* Diagnostics: the table of pipelined-conv instantiations itself, one line per row in the format of fc_debug_conv_routes_read (the thirteen
 * template arguments), copied and counted like that record.  Host code only: it needs no device and no earlier call. */
int fc_debug_conv_table_read(char* buf, int cap);
/* Diagnostics: while the record of fc_debug_conv_routes is on, every launch of the fused linear attention's fast path (n >= 256) adds one
 * line "C n NB TT" to a record of its own: NB = n / 32 and TT = n / 128 when it launched the kernel pair compiled for exactly this shape, 0 0
 * when it launched the pair that reads the shape at run time.  Copies it like fc_debug_conv_routes_read and returns its full length. */
int fc_debug_linattn_routes_read(char* buf, int cap);
/* Diagnostics: while the record of fc_debug_conv_routes is on, every launch at the sampler's step boundary adds one line to a record of its
 * own, in the order the launches were enqueued (a captured graph: when it was captured): "init_conv", "final_conv", or "step_close" for
 * final_res_block's closing convolution on the flavour that stands for both inside a replayed Euler step.  Copies it like
 * fc_debug_conv_routes_read and returns its full length. */
int fc_debug_step_routes_read(char* buf, int cap);
/* Diagnostics: fc_unet_profile_ops runs plan entry `op_index` once more with the stamps of fc_debug_set_conv_stamps going to buf_dev
 * (the phase timeline of ONE launch of a real plan, fused tail included: tools/fin_stamps.py); NULL switches it off. */
int fc_debug_set_stamp_op(int op_index, void* buf_dev);
/* One implicit-GEMM launch on caller tensors (NHWC activations, OIHW weights as torch stores them).
 * Synchronises; allocates a scratch weight buffer. stats_out [B][G][T][2] gets (mean, M2) partials, T and the
 * per-slot count come back through stats_T / stats_nt. tile_cfg = -1 picks automatically.  repeats > 0 additionally
 * times that many back-to-back launches with HIP events (average milliseconds in *ms_out). */
int fc_debug_set_conv_precision(int mode);    /* test hook: arithmetic of fc_debug_conv launches (0 fp32, 1 split-bf16) */
int fc_debug_conv(const float* src0_nhwc, int c0, const float* src1_nhwc, int c1, const float* w_oihw_dev, const float* bias_dev,
                  const float* add_nhwc, float* out_nhwc, float* stats_out, int groups_out, int* stats_T, float* stats_nt, int batch,
                  int hs, int ws, int cout, int ksize, int pad, int stride, int upsample, int out_act, int tile_cfg, int repeats,
                  float* ms_out, void* stream);
/* Tests: `n` weight re-layout jobs as ONE launch of the kernel every plan packs its weights with.  kinds[i]: 0 conv (O, I, KK), 1 space-to-depth
 * conv (O, C), 2 transpose into a slice (R, Cc, ld, col0), 3 copy (n), 4 channel-padded conv (O, I, KK, Opad, Ipad), 5 data-gradient operand
 * (O, I, KS, ci0, nci), 6 k-step-quad conv (O, I, KK), 7 split-bf16 conv (O, I, KK, Ipad), 8 folded upsample (O, I), 9 folded upsample
 * split-bf16 (O, I, Ipad); dims + 5 * i holds job i's dimensions in that order, the rest zero; src[i] / dst[i] are device pointers.
 * dst_floats[i] (or null) receives the size of job i's destination in floats; with src or dst null that is all the call does.  Any other
 * kind: FC_E_ARG, nothing is launched.  Synchronises. */
int fc_debug_pack(int n, const int* kinds, const int* dims, const float* const* src_dev, float* const* dst_dev, int64_t* dst_floats, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Flow training step  (replaces train_flow.py:346-397: interpolation, loss.backward() through flocoder/unet.py,
 * clip_grad_norm_, torch.optim.Adam.step, EMA.update :46-54).  All vectors are caller-owned device memory.
 * ---------------------------------------------------------------------------------------------- */
/* Forward plan (fc_unet_reserve) plus the backward plan over the same arena. */
int fc_unet_train_reserve(fc_unet* u, int max_batch, int height, int width);
/* Gradients of all parameters for the LAST fc_unet_forward(x, time, ids) on this handle (same arguments again), given d(out):
 * grads_flat_dev[numel] in the parameter table's layout (fc_unet_param_info offsets; padding stays zero).  With ids == NULL
 * the class_cond_mlp.* range receives no gradient (zeros); an optimiser must skip it as torch skips p.grad is None. */
int fc_unet_backward(fc_unet* u, const float* x_dev, const float* time_dev, const int64_t* class_ids_dev, const float* d_out_dev,
                     float* grads_flat_dev, int64_t numel, int batch, int height, int width, void* stream);
/* The same with mask conditioning (cond['mask_cond'], unet.py:298-305,336-340,360-364) and the input gradients: mask_dev /
 * mask_is_ones as in fc_unet_forward; dx_out_dev / dmask_out_dev [B,C,H,W] receive d(x) / d(mask) when not NULL (the inpainting
 * step needs both: source and mask reach x through mask_blending, train_flow.py:146-147). */
int fc_unet_backward_ex(fc_unet* u, const float* x_dev, const float* time_dev, const int64_t* class_ids_dev, const float* mask_dev,
                        int mask_is_ones, const float* d_out_dev, float* grads_flat_dev, int64_t numel, float* dx_out_dev,
                        float* dmask_out_dev, int batch, int height, int width, void* stream);
/* The same in two parts, for data-parallel training that overlaps the gradient all-reduce with the backward (train_flow.py:371 under
 * DDP): part 0 runs the data-gradient chain from the output through mid_block1 and every weight / norm / FiLM gradient of final_*,
 * ups.* and mid_*, after which [split_offset, numel) of grads_flat_dev is final (fc_unet_grad_buckets); part 1 runs the rest and completes
 * [0, split_offset).  first_part = 0, last_part = 1 is fc_unet_backward_ex.  Part 1 must follow part 0 of the same forward. */
int fc_unet_backward_parts(fc_unet* u, const float* x_dev, const float* time_dev, const int64_t* class_ids_dev, const float* mask_dev,
                           int mask_is_ones, const float* d_out_dev, float* grads_flat_dev, int64_t numel, float* dx_out_dev,
                           float* dmask_out_dev, int batch, int height, int width, int first_part, int last_part, void* stream);
/* Gradient accumulation: fc_unet_backward_parts with grads_flat_dev[i] += g[i] for every parameter that receives a gradient in this call
 * (g: what fc_unet_backward_parts would have written, by the same arithmetic) and every other element left untouched -- padding, the
 * class_cond_mlp.* range when class_ids_dev == NULL, the mask branches' ranges when they do not run.  Nothing is zeroed; the caller starts
 * a sum with an overwriting backward or a vector it cleared.  dx_out_dev / dmask_out_dev are overwritten as before.  Every element has
 * one writer and the adds follow the stream's order: the same inputs give the same bits run to run.  One optimiser step over more rows
 * than the arena holds = one training forward + one call per micro-batch (d_out scaled by the micro-batch's share of the step,
 * fc_mse_loss_grad_scaled), then fc_grad_clip_coef / fc_adam_ema_step once. */
int fc_unet_backward_accumulate(fc_unet* u, const float* x_dev, const float* time_dev, const int64_t* class_ids_dev, const float* mask_dev,
                                int mask_is_ones, const float* d_out_dev, float* grads_flat_dev, int64_t numel, float* dx_out_dev,
                                float* dmask_out_dev, int batch, int height, int width, int first_part, int last_part, void* stream);
/* Ask for (1) / do without (0, default) the two-bucket form of the backward plan; takes effect at the next fc_unet_train_reserve.  One
 * process gains nothing from it (the deferred table launches run twice); a data-parallel trainer sets it once. */
int fc_unet_set_grad_buckets(fc_unet* u, int on);
/* Number of gradient buckets of the current backward plan (0 none, 1, 2) and the flat offset where the early bucket starts. */
int fc_unet_grad_buckets(const fc_unet* u, int64_t* split_offset);
/* Test hooks: number of entries of the current backward plan (0 before fc_unet_train_reserve), and entry i's kernel family and the
 * reference module it serves -- fc_unet_plan_launches / fc_unet_op_info for the backward plan. */
int fc_unet_backward_launches(const fc_unet* u);
int fc_unet_backward_op_info(const fc_unet* u, int i, const char** kernel, const char** module);
/* 1 when the handle's plans are in the training form fc_unet_train_reserve switches to (they keep every intermediate for the backward; the
 * fused inference launches are not used), else 0.  fc_unet_train_release puts the inference form back: plans and captured graphs are
 * dropped (synchronises the device) and the next fc_unet_reserve builds what a handle that never trained builds, with the same bits. */
int fc_unet_train_form(const fc_unet* u);
int fc_unet_train_release(fc_unet* u);
/* The input gradient alone: d(x) of the LAST training forward for d(out) = d_out_dev, written to dx_out_dev [B,C,H,W].  Same
 * preconditions and FC_E_STATE rule as fc_unet_backward_ex.  Runs the data-gradient chain of the backward plan and nothing whose only
 * products are parameter gradients (weight-gradient launches and tables, their reductions, the activations recomputed for them, the
 * norm / FiLM parameter gradients, the time / class MLP backward): the same kernels in the same order as the full backward, so
 * dx_out_dev has the bits fc_unet_backward_ex would give.  No flat gradient vector is read or written. */
int fc_unet_vjp_x(fc_unet* u, const float* x_dev, const float* time_dev, const int64_t* class_ids_dev, const float* mask_dev,
                  int mask_is_ones, const float* d_out_dev, float* dx_out_dev, int batch, int height, int width, void* stream);
/* Test hooks: the entries of the backward plan fc_unet_vjp_x runs (count; entry i's kernel family and module), as the pair above. */
int fc_unet_vjp_launches(const fc_unet* u);
int fc_unet_vjp_op_info(const fc_unet* u, int i, const char** kernel, const char** module);
/* The backward reads the activations the last training forward left in the handle's single arena.  Every call that writes the arena
 * (fc_unet_forward, fc_unet_integrate, fc_unet_profile_ops, a re-plan by fc_unet_reserve) moves this counter; a caller that keeps
 * several forwards in flight (autograd with two micro-batches, gradient accumulation) compares the value it saw after ITS forward
 * with the current one and re-runs the forward when they differ.  fc_unet_backward[_ex] itself fails with FC_E_STATE when the
 * arena does not hold a training forward of `batch` rows.  (loss.backward() over a graph built earlier, train_flow.py:358-371.) */
uint64_t fc_unet_arena_serial(const fc_unet* u);
/* [lo, hi) of class_cond_mlp.* inside the flat table (0,0 without classes). */
int fc_unet_class_param_range(const fc_unet* u, int64_t* lo, int64_t* hi);
/* x = (1-t) source + t target ; v* = target - source   (train_flow.py:350-353), t per sample.  per_sample (here and in the two
 * calls below) lies in [1, INT_MAX]; anything else is FC_E_ARG. */
int fc_flow_interp(const float* source_dev, const float* target_dev, const float* t_dev, float* x_out_dev, float* v_out_dev, int batch,
                   int64_t per_sample, void* stream);
/* The per-step prologue of train_flow.py:346-357 in one launch: t = warp_time(u (1 - t_eps) + t_eps, s = warp_s) (sampling.py:23-33,
 * the same rounded operations torch runs), time = t * t_scale (the U-Net's time input), x / v* as fc_flow_interp with
 * target row pairing[b] when pairing_dev != NULL (the OT pairing's gather, train_flow.py:350), and the range check of the class ids:
 * bit 0 of *id_flag_dev is set (never cleared) when an id lies outside [0, n_classes) -- nn.Embedding's IndexError, reported when the
 * host next reads the flag; bit 1 when a pairing entry lies outside [0, batch) (torch's target[ot_indices] raises IndexError; the row
 * then reads its own target instead of memory out of bounds).  pairing_dev, class_ids_dev and id_flag_dev may be NULL. */
int fc_flow_prepare(const float* source_dev, const float* target_dev, const int64_t* pairing_dev, const float* u_dev, float t_eps, float warp_s,
                    float t_scale, const int64_t* class_ids_dev, int n_classes, float* t_out_dev, float* time_out_dev, float* x_out_dev,
                    float* v_out_dev, int* id_flag_dev, int batch, int64_t per_sample, void* stream);
/* fc_flow_prepare for rows [first_row, first_row + batch) of a step of target_rows rows (a micro-batch): source_dev, u_dev, class_ids_dev,
 * pairing_dev and the four outputs hold the micro-batch's `batch` rows; target_dev is the WHOLE step's target [target_rows][per_sample],
 * and pairing entries index it: they range over [0, target_rows), bit 1 of *id_flag_dev reports one outside.  Without a pairing row b
 * reads target row first_row + b.  first_row = 0, target_rows = batch is fc_flow_prepare. */
int fc_flow_prepare_rows(const float* source_dev, const float* target_dev, const int64_t* pairing_dev, const float* u_dev, float t_eps, float warp_s,
                         float t_scale, const int64_t* class_ids_dev, int n_classes, float* t_out_dev, float* time_out_dev, float* x_out_dev,
                         float* v_out_dev, int* id_flag_dev, int batch, int first_row, int target_rows, int64_t per_sample, void* stream);
/* A micro-batch's share of a step's MSELoss: dv_out_dev = scale * 2 (v - v*) / numel when not NULL, and *loss_acc_dev += scale *
 * mean((v - v*)^2) (the caller clears the scalar before the first micro-batch).  With scale = rows of the micro-batch / rows of the step
 * the sum over the micro-batches is the whole batch's loss and the accumulated backward its gradient.  ws: 256 floats. */
int fc_mse_loss_grad_scaled(const float* v_dev, const float* target_dev, float* dv_out_dev, float* loss_acc_dev, float* ws256_dev, int64_t numel,
                            float scale, void* stream);
/* loss = mean((v - v*)^2) (train_flow.py:359) and, when dv_out_dev != NULL, its gradient 2 (v - v*) / numel.  ws: 256 floats. */
int fc_mse_loss_grad(const float* v_dev, const float* target_dev, float* dv_out_dev, float* loss_out_dev, float* ws256_dev, int64_t numel,
                     void* stream);
/* clip_grad_norm_ (train_flow.py:392): out[0] = 2-norm over both ranges, out[1] = min(1, max_norm / (norm + 1e-6)).  grads2_dev NULL:
 * one range, numel2 is not looked at.  A negative numel (or numel2 of a second range) is FC_E_ARG. */
int fc_grad_clip_coef(const float* grads_dev, int64_t numel, const float* grads2_dev, int64_t numel2, float max_norm, float* norm_coef_out_dev,
                      float* ws256_dev, void* stream);
/* One torch.optim.Adam step (no weight decay / amsgrad) on grads * (*clip_coef_dev), bias corrections for step count `step`
 * (1-based), followed by ema = decay ema + (1 - decay) p.  apply_adam == 0: EMA only (parameters without a gradient).  The
 * hyper-parameters are doubles, as torch holds them: 1 - beta1, 1 - beta2, lr / bc1, 1 / sqrt(bc2) and 1 - decay are formed in double
 * and rounded to float once each, which is what torch does where a Python scalar meets a float tensor ((float)(1.0 - 0.999) is 0.001f;
 * 1.0f - 0.999f is 1.3e-5 below it).  clip_coef_dev NULL: coefficient 1.  ema_dev NULL: Adam only. */
int fc_adam_ema_step(float* params_dev, const float* grads_dev, float* exp_avg_dev, float* exp_avg_sq_dev, float* ema_dev, int64_t numel,
                     const float* clip_coef_dev, double lr, double beta1, double beta2, double eps, int step, double ema_decay, int apply_adam,
                     void* stream);
/* The same, skipped entirely (no Adam, no EMA) when *skip_flag_dev != 0 (NULL: never): FlowTrainer passes fc_flow_prepare's flag, so a
 * step whose class ids / pairing were out of range changes nothing before the host has seen the flag and raised. */
int fc_adam_ema_step_guarded(float* params_dev, const float* grads_dev, float* exp_avg_dev, float* exp_avg_sq_dev, float* ema_dev, int64_t numel,
                             const float* clip_coef_dev, double lr, double beta1, double beta2, double eps, int step, double ema_decay, int apply_adam,
                             const int* skip_flag_dev, void* stream);
/* test hook: weight / bias gradient of one convolution (NHWC operands, dw in [O][I][KH][KW]) */
int fc_debug_conv_wgrad(const float* src0, int c0, const float* src1, int c1, const float* dy, int cout, int batch, int hs, int ws, int ksize,
                        int pad, int stride, int upsample, float* dw_out, float* db_out, void* stream);
/* The same hook in the forms a training plan uses.  split_target: workgroups wanted per launch (0: the stand-alone default of 1024; the
 * backward plan gives its table entries 256).  accumulate != 0: the gradient is added to what dw_out / db_out hold (the launches of
 * fc_unet_backward_accumulate).  nsplit_out / mtiles_out / tb_out (each may be NULL, host integers): the launch's geometry -- how many
 * workgroups share a 32 x 32 block of dW, how many pixel tiles they walk between them, and how many samples one tile holds. */
int fc_debug_conv_wgrad_ex(const float* src0, int c0, const float* src1, int c1, const float* dy, int cout, int batch, int hs, int ws, int ksize,
                           int pad, int stride, int upsample, float* dw_out, float* db_out, int split_target, int accumulate, int* nsplit_out,
                           int* mtiles_out, int* tb_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SD-VAE codec  (replaces flocoder/codecs.py:631-663 SD_VAE_Wrapper -> diffusers AutoencoderKL, sd-vae-ft-mse config)
 * ---------------------------------------------------------------------------------------------- */
typedef struct fc_vae fc_vae;
/* device >= 0: a gfx950 device; device < 0: description only (parameter table). */
int fc_vae_create(int device, fc_vae** out);
void fc_vae_destroy(fc_vae* v);
/* Parameter table: names/shapes are the upstream AutoencoderKL state_dict keys ("encoder.conv_in.weight", ...). */
int fc_vae_param_count(const fc_vae* v);
int64_t fc_vae_param_numel(const fc_vae* v);
int fc_vae_param_info(const fc_vae* v, int i, const char** name, int64_t shape[4], int64_t* offset);
int fc_vae_load_params(fc_vae* v, const float* flat, int64_t numel, int on_device, void* stream);
/* Plans + arenas.  Images HxW (powers of two >= 64), latents (H/8)x(W/8). */
int fc_vae_reserve_encode(fc_vae* v, int max_batch, int height, int width);
int fc_vae_reserve_decode(fc_vae* v, int max_batch, int lat_height, int lat_width);
/* mean = vae.encode(x).latent_dist.mean  (codecs.py:642): x_dev [B,3,H,W] -> mean_out_dev [B,4,H/8,W/8]; no scaling factor. */
int fc_vae_encode(fc_vae* v, const float* x_dev, float* mean_out_dev, int batch, int height, int width, void* stream);
/* x = vae.decode(z).sample  (codecs.py:651): z_dev [B,4,h,w] -> x_out_dev [B,3,8h,8w]. */
int fc_vae_decode(fc_vae* v, const float* z_dev, float* x_out_dev, int batch, int lat_height, int lat_width, void* stream);
/* Arithmetic of the plans built from now on: 0 = exact fp32 (default; what every parity test and the headline benchmark use), 1 = split-bf16
 * -- each fp32 operand as bf16 hi + lo, a product as hi*hi + hi*lo + lo*hi on the bf16 matrix pipe with fp32 accumulation (~1e-5 relative per
 * layer): an OPT-IN for callers that decode many images and accept that (sampling.py:150-183 decode_latents).  No counterpart upstream.
 * Changing the mode drops the current plans. */
int fc_vae_set_precision(fc_vae* v, int mode);
double fc_vae_flops_per_sample(const fc_vae* v, int decode);
int fc_vae_plan_launches(const fc_vae* v, int decode);
/* Measurement only: launch i of the encode / decode plan, and every launch timed alone (see fc_unet_profile_ops). */
int fc_vae_op_info(const fc_vae* v, int decode, int i, const char** kernel, const char** module, double* flops_per_sample);
int fc_vae_profile_ops(fc_vae* v, int decode, const float* in_dev, float* out_dev, int batch, int repeats, float* ms_out, int n_out,
                       void* stream);
int fc_vae_op_bytes(const fc_vae* v, int decode, int i, double* bytes_per_sample, double* bytes_per_launch);   /* as fc_unet_op_bytes */
/* Tests only.  on != 0: the plans built from now on recycle no activation buffer and record their tensors by reference module name
 * ("decoder.mid_block.resnets.0", its conv1 output ".h1", an attention's ".q .k .v .p .o", ...); the arena grows to the sum of all tensors
 * (~1 GB for one 256x256 decode).  Changing the switch drops the current plans; with it off nothing differs from a handle that never had it.
 * fc_*_debug_tensor: the NHWC tensor [max_batch][H][W][C] the encode (decode = 0) / decode plan recorded under `name`, as the last run left it
 * (copy it with fc_debug_copy). */
int fc_vae_debug_taps(fc_vae* v, int on);
int fc_vae_debug_tensor(const fc_vae* v, int decode, const char* name, const float** ptr, int* channels, int* height, int* width);

/* ------------------------------------------------------------------------------------------------
 * VQVAE codec, encode / decode  (replaces flocoder/codecs.py:386-525 VQVAE.encode / VQVAE.decode with
 * EncDecResidualBlock :150-214, AttnBlock :53-89, Decoder :217-316, SpatialNonLocalAttention :337-383; no NATTEN, eval)
 * quantize() (third-party ResidualVQ) is not part of this library.
 * ---------------------------------------------------------------------------------------------- */
typedef struct fc_vqvae fc_vqvae;
/* Constructor arguments of VQVAE (codecs.py:399-405); widths must be multiples of 4.  device < 0: description only. */
int fc_vqvae_create(int in_channels, int hidden_channels, int num_downsamples, int internal_dim, int vq_embedding_dim, int decoder_nonlocal,
                    int device, fc_vqvae** out);
/* The same with NATTENBlocks (codecs.py:93-145; 7x7 neighbourhood attention, 8 heads) in the EncDecResidualBlocks the reference
 * gives them to when the natten package is importable: the last two encoder levels, the bottleneck block, the first decoder block
 * (decoder_nonlocal == 0) and the first upsampling level (codecs.py:266,275-278,414-429).  natten_layout: 0 = none (fc_vqvae_create),
 * 1 = windows over image rows x columns per head (the intended reading), 2 = what natten >= 0.20 computes from the reference's
 * [B, heads, H, W, d] tensors (windows over head index x image rows, per image column).  PARITY UNPINNED: the package is absent. */
int fc_vqvae_create_ex(int in_channels, int hidden_channels, int num_downsamples, int internal_dim, int vq_embedding_dim,
                       int decoder_nonlocal, int natten_layout, int device, fc_vqvae** out);
/* 2-D neighbourhood attention by itself: qkv_nhwc_dev [B][H][W][3C] (channel = which*C + head*(C/heads) + d), out [B][H][W][C],
 * kernel_size odd <= 7, windows clamped (shifted) at the borders, scale (C/heads)^-0.5, optional scalar gate gamma_dev[0].
 * Replaces natten.functional.na2d / na2d_qk + softmax + na2d_av (codecs.py:130-135). */
int fc_na2d(const float* qkv_nhwc_dev, float* out_nhwc_dev, const float* gamma_dev, int batch, int height, int width, int channels,
            int heads, int kernel_size, int layout_mode, void* stream);
void fc_vqvae_destroy(fc_vqvae* v);
/* Parameter table: the reference's state_dict keys ("encoder.0.conv1.weight", "decoder.layers.0.q_proj.weight", ...). */
int fc_vqvae_param_count(const fc_vqvae* v);
int64_t fc_vqvae_param_numel(const fc_vqvae* v);
int fc_vqvae_param_info(const fc_vqvae* v, int i, const char** name, int64_t shape[4], int64_t* offset);
int fc_vqvae_load_params(fc_vqvae* v, const float* flat, int64_t numel, int on_device, void* stream);
/* Plans + arenas.  Images HxW (powers of two), latents (H >> num_downsamples) x (W >> num_downsamples), >= 4 per side. */
int fc_vqvae_reserve_encode(fc_vqvae* v, int max_batch, int height, int width);
int fc_vqvae_reserve_decode(fc_vqvae* v, int max_batch, int lat_height, int lat_width);
/* z = vqvae.encode(x)  (codecs.py:492-502): x_dev [B,in_channels,H,W] -> z_out_dev [B,vq_embedding_dim,h,w] (pre-quantisation). */
int fc_vqvae_encode(fc_vqvae* v, const float* x_dev, float* z_out_dev, int batch, int height, int width, void* stream);
/* x = vqvae.decode(z_q)  (codecs.py:523-525, noise_strength 0): z_dev [B,vq_embedding_dim,h,w] -> x_out_dev [B,in_channels,H,W]. */
int fc_vqvae_decode(fc_vqvae* v, const float* z_dev, float* x_out_dev, int batch, int lat_height, int lat_width, void* stream);
int fc_vqvae_set_precision(fc_vqvae* v, int mode);     /* as fc_vae_set_precision */
int fc_vqvae_debug_taps(fc_vqvae* v, int on);          /* as fc_vae_debug_taps: block outputs by state_dict prefix, ".h1 .mid .h2 .res" ... */
int fc_vqvae_debug_tensor(const fc_vqvae* v, int decode, const char* name, const float** ptr, int* channels, int* height, int* width);
double fc_vqvae_flops_per_sample(const fc_vqvae* v, int decode);
/* Measurement only (bench.py's config-5 leg): launches of the encode / decode plan, launch i's kernel family, module, algorithmic FLOPs
 * per sample and HBM bytes (per sample / per launch; 0 where not stated), and every launch timed alone as in fc_unet_profile_ops. */
int fc_vqvae_plan_launches(const fc_vqvae* v, int decode);
int fc_vqvae_op_info(const fc_vqvae* v, int decode, int i, const char** kernel, const char** module, double* flops_per_sample,
                     double* bytes_per_sample, double* bytes_per_launch);
int fc_vqvae_profile_ops(fc_vqvae* v, int decode, const float* in_dev, float* out_dev, int batch, int repeats, float* ms_out, int n_out,
                         void* stream);
/* z_q, indices = ResidualVQ(z) in inference form (replaces VQVAE.quantize, codecs.py:504-521 -> vector_quantize_pytorch.ResidualVQ,
 * third party, parity unpinned): per level the nearest codeword of the running residual, z_q = their sum.
 * z_dev / zq_out_dev [B,dim,hw] (NCHW with hw = h*w); codebooks_dev [levels][codebook_size][dim]; indices_out_dev [B*hw][levels]
 * int64 or NULL. */
int fc_rvq_quantize(const float* z_dev, const float* codebooks_dev, float* zq_out_dev, int64_t* indices_out_dev, int batch, int dim, int hw,
                    int codebook_size, int levels, void* stream);

/* Fitting the quantiser's codebooks on the device without gradients (the EMA / k-means / dead-code form of
 * vector_quantize_pytorch's codebook as the reference configures it, codecs.py:456-467; third party, parity unpinned; the definition is
 * DESIGN.md section 4 "Codebook fitting", its host form flocoder_amd/noise.py codebook_*).  Tensors as fc_rvq_quantize: z_dev [B,dim,hw],
 * codebooks_dev [levels][codebook_size][dim], indices [B*hw][levels] int64; cluster_size_dev [levels][codebook_size] and embed_avg_dev
 * [levels][codebook_size][dim] fp32.  Supported: dim <= 16, codebooks <= 64 KB, B*hw <= 2^24; anything else FC_E_SHAPE.  Every call
 * assigns with the search of fc_rvq_quantize, accumulates counts as integers and sums as 64-bit fixed point (integer atomics: the same
 * bits run to run; error bound at the head of csrc/rvq_train.hip), enqueues on `stream`, allocates nothing and reads nothing back;
 * ws_dev is caller-owned scratch of fc_rvq_train_workspace_bytes(...) bytes (0 for an unsupported shape), 64-byte aligned.
 *
 * fc_codebook_draws: out_dev [count] int64, slot j = pi(j mod n), pi the permutation of [0, n) of (seed, level, draw_index): Philox4x32-10
 * under key seed + FC_CODEBOOK_KEY_OFFSET (mod 2^64), counter (0 | 1, draw_index, level, n), keys a bijection of [0, 2^b) (four rounds of
 * an odd multiply-add and a xor-shift) that is cycle-walked into [0, n).
 * fc_rvq_seed_codes: code slot j of `level` <- the residual entering that level of vector pi(j), j = 0 .. codebook_size-1 (levels below
 * it are read, nothing else is written).
 * fc_rvq_kmeans: `iters` Lloyd iterations of `level` on the residuals entering it, means in place in the codebook; an empty cluster keeps
 * its mean.  cluster_size_out_dev [codebook_size] / embed_avg_out_dev [codebook_size][dim] (both or neither): the last iteration's counts
 * and mean * count (zeros for iters = 0).  objective_out_dev NULL or [iters] fp64: iteration i's sum of squared distances of the
 * residuals to the means they were assigned to (before that iteration's update).  1 + 2 iters launches, iters memsets.
 * fc_rvq_train_step: all levels assign against the codebooks as passed (zq_out_dev / indices_out_dev are fc_rvq_quantize's of them, bit
 * for bit), then in place cluster_size <- cs + (1-decay)(n - cs), embed_avg likewise with the sums, codebook <- embed_avg / Laplace-smoothed
 * cluster size, and with threshold_ema_dead_code > 0 the j-th code in index order below it <- residual of vector pi(j), its cluster
 * size the threshold, its embed_avg codeword * threshold.  losses_out_dev [levels] fp32: commitment_weight * mean squared distance;
 * expired_out_dev [levels] int32.  Three launches and one memset. */
#define FC_CODEBOOK_KEY_OFFSET 0x43424F4F4B464954ULL /* "CBOOKFIT" */
size_t fc_rvq_train_workspace_bytes(int batch, int hw, int dim, int codebook_size, int levels);
int fc_codebook_draws(int64_t* out_dev, uint64_t seed, int level, int64_t draw_index, int64_t n, int64_t count, void* stream);
int fc_rvq_seed_codes(const float* z_dev, float* codebooks_dev, int batch, int dim, int hw, int codebook_size, int levels, int level, uint64_t seed,
                      int64_t draw_index, void* stream);
int fc_rvq_kmeans(const float* z_dev, float* codebooks_dev, int batch, int dim, int hw, int codebook_size, int levels, int level, int iters,
                  float* cluster_size_out_dev, float* embed_avg_out_dev, double* objective_out_dev, void* ws_dev, size_t ws_bytes, void* stream);
int fc_rvq_train_step(const float* z_dev, float* codebooks_dev, float* cluster_size_dev, float* embed_avg_dev, float* zq_out_dev,
                      int64_t* indices_out_dev, float* losses_out_dev, int* expired_out_dev, int batch, int dim, int hw, int codebook_size,
                      int levels, double decay, double commitment_weight, float threshold_ema_dead_code, uint64_t seed, int64_t draw_index,
                      void* ws_dev, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Inpainting conditioning  (replaces flocoder/inpainting.py:161-253 MaskEncoder / mask_blending)
 * ---------------------------------------------------------------------------------------------- */
typedef struct fc_mask_encoder fc_mask_encoder;
int fc_mask_encoder_create(int device, fc_mask_encoder** out);        /* device < 0: description only */
void fc_mask_encoder_destroy(fc_mask_encoder* m);
int fc_mask_encoder_param_count(const fc_mask_encoder* m);            /* names: "layers.0.conv1.weight", ... */
int64_t fc_mask_encoder_param_numel(const fc_mask_encoder* m);
int fc_mask_encoder_param_info(const fc_mask_encoder* m, int i, const char** name, int64_t shape[4], int64_t* offset);
int fc_mask_encoder_load_params(fc_mask_encoder* m, const float* flat, int64_t numel, int on_device, void* stream);
int fc_mask_encoder_reserve(fc_mask_encoder* m, int max_batch, int height, int width);
/* MaskEncoder.forward (inpainting.py:235-245): mask_pixels_dev [B,1,H,W] fp32 -> mask_latents_dev [B,4,H/16,W/16]. */
int fc_mask_encoder_forward(fc_mask_encoder* m, const float* mask_pixels_dev, float* mask_latents_dev, int batch, int height, int width,
                            void* stream);
/* Parameter gradients of the LAST fc_mask_encoder_forward on this object (same mask_pixels again, its output in mask_latents_dev)
 * for d(mask_latents): grads_flat_dev[numel] in the parameter-table layout, overwritten or (accumulate != 0) added to.  Replaces
 * the MaskEncoder leg of loss.backward() in the inpainting step (train_flow.py:312-318,361-371). */
int fc_mask_encoder_backward(fc_mask_encoder* m, const float* mask_pixels_dev, const float* mask_latents_dev, const float* d_latents_dev,
                             float* grads_flat_dev, int64_t numel, int accumulate, int batch, int height, int width, void* stream);
/* mask_blending (inpainting.py:250-253): out = source + mask * (noise - source), elementwise over numel floats. */
int fc_mask_blend(const float* source_dev, const float* mask_dev, const float* noise_dev, float* out_dev, int64_t numel, void* stream);

/* ------------------------------------------------------------------------------------------------
 * OT pairing  (replaces flocoder/ot.py:63-84 compute_ot_pairing)
 * ---------------------------------------------------------------------------------------------- */
/* The greedy matcher.  source_dev/target_dev [B,D] fp32; dist_ws_dev workspace of B*B floats; perm_out_dev [B] int64. */
int fc_ot_pairing(const float* source_dev, const float* target_dev, int batch, int64_t dim, float* dist_ws_dev,
                  int64_t* perm_out_dev, void* stream);
/* Exact mini-batch OT pairing: perm minimises sum_i |s_i - t_perm[i]|^2 over permutations.  cost_ws_dev: B*B floats, holds the
 * squared-distance matrix on return; duals_out_dev: NULL or 2*B doubles (u then v) with u_i + v_j <= c_ij, equality on the pairing. */
int fc_ot_pairing_exact(const float* source_dev, const float* target_dev, int batch, int64_t dim, float* cost_ws_dev,
                        int64_t* perm_out_dev, double* duals_out_dev, void* stream);
/* The solver alone on a caller's cost matrix cost_dev [B][B] fp32 (non-finite entries count as FLT_MAX). */
int fc_ot_assign(const float* cost_dev, int batch, int64_t* perm_out_dev, double* duals_out_dev, void* stream);

/* Entropic (Sinkhorn) plans between uniform marginals, 1 <= batch <= 1024.  Everything below runs on `stream`, allocates nothing and
 * never synchronises.
 *
 * fc_ot_sinkhorn: the log-domain Sinkhorn-Knopp iteration on cost_dev [B][B] fp32 (non-finite entries count as FLT_MAX):
 *     f = g = reg log(1/B);  per iteration  g_j = reg (log(1/B) - LSE_i((f_i - C_ij)/reg)),  f_i = reg (log(1/B) - LSE_j((g_j - C_ij)/reg));
 *     after every 10th iteration err = | colsum(P) - 1/B |_2 with P_ij = exp((f_i + g_j - C_ij)/reg); stop when err < stop_thr or at max_iter.
 * reg > 0, stop_thr >= 0, 1 <= max_iter <= 10000 (rounded up to a multiple of 10), else FC_E_ARG.  POT's defaults: 1000, 1e-9.
 * plan_out_dev [B][B] fp32 (row sums 1/B to rounding: the row half comes last); duals_out_dev 2*B doubles, f then g;
 * info_out_dev 3 doubles: {iterations run, converged (1.0 / 0.0), err at the last check}. */
int fc_ot_sinkhorn(const float* cost_dev, int batch, double reg, int max_iter, double stop_thr, float* plan_out_dev, double* duals_out_dev,
                   double* info_out_dev, void* stream);
/* The plan between source_dev / target_dev [B,D] fp32 under the squared Euclidean cost; normalize_cost != 0 divides the matrix by its
 * largest entry first (torchcfm's option; FLT_MAX sentinels are left out of the maximum and of the division, an all-zero matrix is left
 * alone).  cost_ws_dev: B*B floats, the matrix the solver saw on return; the other outputs as fc_ot_sinkhorn. */
int fc_ot_plan_sinkhorn(const float* source_dev, const float* target_dev, int batch, int64_t dim, double reg, int normalize_cost, int max_iter,
                        double stop_thr, float* plan_out_dev, double* duals_out_dev, double* info_out_dev, float* cost_ws_dev, void* stream);
/* n_pairs (1 .. 65536) index pairs drawn with replacement from plan_dev [B][B] read as a categorical over its cells (torchcfm's
 * sample_map): pair k inverts the two-level fp64 cdf at the 53-bit uniform of Philox4x32-10 block (counter (k, draw_index, 0x4F54504C,
 * 0xFFFFFFFF), key = seed); flocoder_amd/noise.py plan_uniforms is the host form.  i_out_dev / j_out_dev [n_pairs] int64.  A plan whose
 * sum is not positive and finite gives the pairs (k mod B, k mod B) and sets *info_dev = 1 (info_dev may be NULL; never cleared here). */
int fc_ot_sample_plan(const float* plan_dev, int batch, int n_pairs, uint64_t seed, uint32_t draw_index, int64_t* i_out_dev, int64_t* j_out_dev,
                      int* info_dev, void* stream);
/* A plan as a permutation (upstream's compute_ot_pairing_vanilla): for rows in order the largest entry among the unused columns, ties to
 * the lowest column. */
int fc_ot_plan_pairing(const float* plan_dev, int batch, int64_t* perm_out_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Parity metrics  (replace flocoder/metrics.py:40-54 sinkhorn_loss: geomloss SamplesLoss("sinkhorn", p=2, blur=0.05))
 * ---------------------------------------------------------------------------------------------- */
/* Debiased Sinkhorn divergence S_eps(x, y) between the point clouds x_dev [n][dim] and y_dev [m][dim] (fp32, uniform weights),
 * cost |x-y|^2/2, eps-scaling from diameter^2 down to blur^2 by factors scaling^2 (geomloss's tensorized algorithm, restated:
 * PARITY UNPINNED, the package is absent).  diameter <= 0: computed from the data as geomloss does.  Results on the host
 * (the call synchronises `stream`): *value_out_host, the diameter used, the number of eps steps.  n, m <= 8192. */
int fc_sinkhorn_divergence(const float* x_dev, const float* y_dev, int n, int m, int64_t dim, double blur, double scaling,
                           double diameter, double* value_out_host, double* diameter_out_host, int* iterations_out_host,
                           void* stream);

/* ------------------------------------------------------------------------------------------------
 * Nearest neighbours  (no upstream counterpart: exact k-NN over latent sets, the primitive under metrics.prdc)
 * ---------------------------------------------------------------------------------------------- */
/* d2(a, b) = sum_f (a_f - b_f)^2 in fp32 by direct differences, one accumulator per pair over the features in ascending order,
 * acc = fma(a_f - b_f, a_f - b_f, acc): a function of the two vectors alone (the same bits whichever is the query and whichever tile,
 * chunk, batch or call the pair falls in); a non-finite d2 is stored as FLT_MAX.  Neighbours are ordered by (d2, global reference
 * index), ties to the lower index.  1 <= k <= 64, dim >= 1, 1 <= n_query <= 2^30, n_ref >= 0, first_index >= 0, else FC_E_SHAPE; null
 * or misaligned pointers FC_E_ARG.  A dim that is not a multiple of 4, or q_dev / ref_dev not 16-byte aligned, takes scalar loads.
 * Everything runs on `stream`, allocates nothing, reads nothing back and never waits for another workgroup.
 *
 * fc_knn_update merges the references ref_dev [n_ref][dim] of global indices first_index .. first_index + n_ref - 1 into the running
 * lists best_d2_inout_dev / best_idx_inout_dev [n_query][k], ascending, empty slots (+inf, -1) -- which is how the caller initialises
 * them.  query_ids_dev (may be NULL) [n_query]: the reference whose global index equals query_ids[q] is skipped for query q.  Any split
 * of the references into calls, in any order, gives the same bits as one call.  ws_dev: 16-byte aligned, the workspace-bytes function's
 * size for the same (n_query, n_ref, k).
 * fc_knn_ball_counts: counts_inout_dev[q] += #{r : d2(q, r) <= radius2_dev[r]} over the same references (radius2_dev [n_ref], one per
 * reference row of this call; integer atomics, so the result does not depend on their order). */
int64_t fc_knn_workspace_bytes(int n_query, int64_t n_ref, int k);
int fc_knn_update(const float* q_dev, int n_query, const float* ref_dev, int64_t n_ref, int64_t dim, int k, int64_t first_index,
                  const int64_t* query_ids_dev, float* best_d2_inout_dev, int64_t* best_idx_inout_dev, void* ws_dev, void* stream);
int fc_knn_ball_counts(const float* q_dev, int n_query, const float* ref_dev, int64_t n_ref, int64_t dim, const float* radius2_dev,
                       int64_t first_index, const int64_t* query_ids_dev, int32_t* counts_inout_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Set distances  (no upstream counterpart: Frechet and kernel (KID) distances between sample sets)
 * ---------------------------------------------------------------------------------------------- */
#define FC_JACOBI_LDS_R 4088        /* longest vector a pair of which stays in LDS between the products and the rotation */
#define FC_JACOBI_MAX_SWEEPS 30
#define FC_FRECHET_MAX_SMALL 4096   /* min(n1, n2), and the number of vectors of a Jacobi solve */
#define FC_FRECHET_MAX_LARGE 16384  /* max(n1, n2) */
#define FC_GRAM_MAX_ROWS 65536
#define FC_WS_GRAM 0
#define FC_WS_MOMENTS 1
#define FC_WS_JACOBI 2
#define FC_WS_FRECHET 3
#define FC_WS_KID 4
#define FC_WS_MOMENTS_UPDATE 5      /* the moment form's workspaces: dim as given, n1 and n2 are not looked at beyond 1 .. 65536 */
#define FC_WS_MOMENTS_MERGE 6
#define FC_WS_MOMENTS_FACTOR 7
#define FC_WS_MOMENTS_DISTANCE 8
/* Sets are fp32 [rows][dim] row-major on the device; every result is fp64.  All sums run in a fixed order (per-workgroup partials added by a
 * second launch, no floating-point atomics): the same bits run to run.  Everything runs on `stream` and allocates nothing; workspaces
 * are the caller's, 16-byte aligned, of the workspace-bytes function's size for the kind (FC_WS_*) and the call's own n1, n2, dim
 * (FC_WS_MOMENTS: n1 = n2 = n; FC_WS_JACOBI: n1 = n, n2 = r).  Limits -> FC_E_SHAPE, null or misaligned pointers -> FC_E_ARG, both before any launch.
 *
 * fc_gram_f64: c_out_dev [n1][n2] = scale * sum_f (a[i][f] - mean_a[f]) (b[j][f] - mean_b[f]); the means are [dim] fp64 or NULL (no
 *   centring), subtracted in fp64 on load; products and sums on the fp64 matrix pipe.  fro2_out_dev (NULL, or one fp64; then ws_dev of
 *   FC_WS_GRAM): the squared Frobenius norm of the stored matrix.  1 <= n1, n2 <= 65536, dim >= 1.
 * fc_col_moments: mean_out_dev [dim] = the mean of every feature, *ssq_out_dev = sum_i |x_i - mean|^2.  ws_dev: FC_WS_MOMENTS.
 * fc_jacobi_svals: the singular values of the fp64 matrix given as n vectors of r contiguous elements (z_inout_dev [n][r], destroyed), by
 *   one-sided Jacobi: sweeps of n' - 1 rounds of the round-robin schedule (n' = n rounded up to even; the padding vector is zero and its
 *   pairs do nothing), one launch per round, one workgroup per pair.  A pair with alpha = |a|^2, beta = |b|^2, gamma = a.b (recomputed
 *   every time) is left alone when |gamma| <= r 2^-53 sqrt(alpha beta) or alpha beta <= (2^-53 ||Z||_F^2)^2, else rotated by the
 *   smaller-angle tangent.  The host reads one 8-byte word per sweep (rotations, non-finite pairs) and stops after the first sweep
 *   without a rotation (*converged_out_host = 1), after a sweep that met a non-finite product, or after FC_JACOBI_MAX_SWEEPS (0).
 *   svals_out_dev [n]: the vector norms, descending; nuclear_out_dev (may be NULL): their sum.  1 <= n <= 4096, r >= 1.
 * fc_frechet_sets: out_dev [6] = {FD, |mx - my|^2, tr S1, tr S2, ||C||_*, ||C||_F^2} with
 *   FD = |mx - my|^2 + sum |x - mx|^2 / (n1 - 1) + sum |y - my|^2 / (n2 - 1) - 2 ||C||_*, C = the centred cross-Gram of the smaller set
 *   against the larger, scaled by 1 / sqrt((n1 - 1)(n2 - 1)) -- tr sqrt(S1 S2) = ||C||_* exactly, and no dim x dim matrix is formed.
 *   svals_out_dev: NULL or [min(n1, n2)].  launches_out_host: NULL or the number of kernel launches of the call.
 *   2 <= n1, n2; min(n1, n2) <= 4096; max(n1, n2) <= 16384; dim >= 1.
 * fc_kid_sets: out_dev [4] = {MMD^2, sum_{i != j} k(x_i, x_j), sum_{i != j} k(y_i, y_j), sum_{i, j} k(x_i, y_j)}, k(x, y) = (x.y / dim + 1)^3,
 *   MMD^2 = sum_xx / (n1 (n1 - 1)) + sum_yy / (n2 (n2 - 1)) - 2 sum_xy / (n1 n2): three Gram launches whose epilogue reduces.
 *   2 <= n1, n2 <= 16384.
 *
 * The moment form of the Frechet distance, for sets with far more samples than features (1 <= dim <= 4096).  The state of a set is its
 * sample count (the caller's, on the host), mean [dim] and M [dim][dim] = sum_i (x_i - mean)(x_i - mean)^T, fp64, full and bit-symmetric.
 * fc_frechet_moments_update: takes the batch x_dev [nb][dim] into a state of n_before samples by Chan's pairwise rule: with mean_b and
 *   M_b the batch's own mean and centred scatter (fp32 rows centred in fp64 on load, fp64 matrix pipe, lower-triangle tiles, each tile
 *   and its mirror written by one workgroup), d = mean_b - mean and N = n_before + nb: M += M_b + (n_before nb / N) d d^T,
 *   mean += (nb / N) d.  n_before = 0 stores instead (mean and M need no initialisation).  1 <= nb <= 65536.  ws_dev: FC_WS_MOMENTS_UPDATE.
 * fc_frechet_moments_merge: the same rule with the second state (n_b >= 1, mean_b, m_b) in the batch's place; n_a = 0 copies.
 *   ws_dev: FC_WS_MOMENTS_MERGE.
 * fc_frechet_moments_factor: from a state of n >= 2 samples, S = M / (n - 1): factor_out_dev [dim][dim] = F with F^T F = S (the rows
 *   of S rotated by fc_jacobi_svals' iteration until orthogonal, z_i = lambda_i v_i^T, each divided by the square root of its norm;
 *   zero rows stay zero; row order is the iteration's), evals_out_dev [dim] = the row norms = the eigenvalues of S, descending,
 *   *trace_out_dev = tr S (the diagonal's sum).  sweeps / converged as fc_jacobi_svals.  ws_dev: FC_WS_MOMENTS_FACTOR.
 * fc_frechet_moments_distance: out_dev [6] = {FD, |m1 - m2|^2, tr S1, tr S2, ||F1 F2^T||_*, ||F1 F2^T||_F^2},
 *   FD = |m1 - m2|^2 + tr S1 + tr S2 - 2 ||F1 F2^T||_* (tr sqrt(S1 S2) = ||F1 F2^T||_*): one dim x dim fp64 Gram of the two factors' rows
 *   and one Jacobi solve.  trace1_dev / trace2_dev: one fp64 each, as fc_frechet_moments_factor left them.  svals_out_dev: NULL or
 *   [dim].  ws_dev: FC_WS_MOMENTS_DISTANCE. */
int64_t fc_frechet_workspace_bytes(int what, int n1, int n2, int64_t dim);
int fc_gram_f64(const float* a_dev, int n1, const float* b_dev, int n2, int64_t dim, const double* mean_a_dev, const double* mean_b_dev,
                double scale, double* c_out_dev, double* fro2_out_dev, void* ws_dev, void* stream);
int fc_col_moments(const float* x_dev, int n, int64_t dim, double* mean_out_dev, double* ssq_out_dev, void* ws_dev, void* stream);
int fc_jacobi_svals(double* z_inout_dev, int n, int r, double* svals_out_dev, double* nuclear_out_dev, void* ws_dev, int* sweeps_out_host,
                    int* converged_out_host, void* stream);
int fc_frechet_sets(const float* x_dev, int n1, const float* y_dev, int n2, int64_t dim, void* ws_dev, double* out_dev, double* svals_out_dev,
                    int* sweeps_out_host, int* converged_out_host, int64_t* launches_out_host, void* stream);
int fc_kid_sets(const float* x_dev, int n1, const float* y_dev, int n2, int64_t dim, void* ws_dev, double* out_dev, void* stream);
int fc_frechet_moments_update(const float* x_dev, int nb, int dim, int64_t n_before, double* mean_inout_dev, double* m_inout_dev, void* ws_dev,
                              void* stream);
int fc_frechet_moments_merge(int dim, int64_t n_a, double* mean_a_inout_dev, double* m_a_inout_dev, int64_t n_b, const double* mean_b_dev,
                             const double* m_b_dev, void* ws_dev, void* stream);
int fc_frechet_moments_factor(int dim, int64_t n, const double* m_dev, double* factor_out_dev, double* evals_out_dev, double* trace_out_dev,
                              void* ws_dev, int* sweeps_out_host, int* converged_out_host, int64_t* launches_out_host, void* stream);
int fc_frechet_moments_distance(int dim, const double* mean1_dev, const double* factor1_dev, const double* trace1_dev, const double* mean2_dev,
                                const double* factor2_dev, const double* trace2_dev, void* ws_dev, double* out_dev, double* svals_out_dev,
                                int* sweeps_out_host, int* converged_out_host, int64_t* launches_out_host, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Piano rolls and MIDI  (flocoder/pianoroll.py: img2midi_multi, and the painting of get_piano_rolls + piano_roll_to_img; DESIGN.md
 * section 4 "Piano rolls and MIDI"; the definitions are flocoder_amd/pianoroll.py's NumPy functions)
 * ---------------------------------------------------------------------------------------------- */
#define FC_ROLL_STRIPS 0            /* [B,3,128 S,W]: column t = s W + x reads pixel (128 s + y, x) */
#define FC_ROLL_SQUARE 1            /* 256 x 256: t < 256 reads (y, t), t >= 256 reads (128 + y, 511 - t) */
#define FC_ROLL_GRID 2              /* 2048 x 2048: 64 squares, row-major, 512 columns each */
#define FC_ROLL_MAX_COLUMNS 32768
#define FC_ROLL_MAX_WIDTH 2048
/* Integer work only, on `stream`, nothing allocated, nothing waited for, no atomic decides a note's place: the same bits run to run.
 * fc_pianoroll_scan: images_dev uint8 (is_float = 0) or fp32 (1; read through metrics.to_uint8's per-image stretch, NaN as 0)
 *   [batch][3][height][width]; classifies, runs the onset scan (require_onsets), zeroes rows 0 / 127 of every strip, draws the separators
 *   (every `separators` columns, 0 = none) and leaves in ws_dev (16-byte aligned, fc_pianoroll_workspace_bytes(batch, columns)) the velocity
 *   plane and the note masks; counts_out_dev [batch] = the number of notes of every roll.  split_on_onsets: a red pixel behind a sounding
 *   column also ends the running note and starts another.
 * fc_pianoroll_emit: from the workspace of a scan of the same batch and columns, notes_out_dev int32 [batch][max_notes][4] = (pitch,
 *   start, end, velocity) ascending in (end, pitch), the first max_notes of every roll, the rest -1.  16-byte aligned.
 * fc_pianoroll_render: notes_dev [batch][max_notes][4] + counts_dev [batch] (entries at or past min(count, max_notes) are not read) ->
 *   images_out_dev uint8 [batch][3][128][width], columns col0_dev[b] (NULL: 0) .. + width of the roll in which every entry in list order
 *   sets [start, end) of its pitch to its velocity (clamped to 0..255) and then column start - 1 to 0; green = min(2 v, 255), a pixel is
 *   red (g, 0, 0) iff v >= 11 and (t = 0 or v[t - 1] <= 9), else (0, g, 0); image row 127 - pitch.  Entries with a pitch outside 0..127
 *   paint nothing. */
int64_t fc_pianoroll_workspace_bytes(int batch, int columns);   /* -1: outside the limits */
int fc_pianoroll_scan(const void* images_dev, int is_float, int batch, int height, int width, int layout, int require_onsets, int separators,
                      int split_on_onsets, void* ws_dev, int64_t* counts_out_dev, void* stream);
int fc_pianoroll_emit(const void* ws_dev, int batch, int columns, int32_t* notes_out_dev, int max_notes, void* stream);
int fc_pianoroll_render(const int32_t* notes_dev, const int64_t* counts_dev, int batch, int max_notes, int width, const int32_t* col0_dev,
                        uint8_t* images_out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLOCODER_AMD_H */
