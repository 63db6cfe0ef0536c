// ODE integrator state updates (sampling.py:36-48 rk4_step, :69-74 CFG blend; legacy Euler
// train_sd_flowers.py:58-64).  The state lives in the reference's NCHW boundary layout; every op is a
// single rounded fp32 operation in the reference's order (no FMA contraction), so the only differences
// against the CPU path come from the U-Net itself.
//
// rk4_step's state arithmetic is written once (stage_t, rk4_stage_state, rk4_comb4) and used by every kernel that closes a stage or an
// interval: ode_rk4_stage_kernel / ode_rk4_final_kernel (one template each, plain and measurement-guided) and the likelihood pair
// ode_ll_stage_kernel / ode_ll_final_kernel, which differs in its partition (one workgroup per sample), not in its arithmetic.
#include "common.h"
#include "philox.h"

namespace fc {

__device__ __forceinline__ float mul_(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add_(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float sub_(float a, float b) { return __fsub_rn(a, b); }

// v_no_class + cfg * (v - v_no_class), sampling.py:74
__device__ __forceinline__ float cfg_blend(float vc, float vn, float cfg) { return add_(vn, mul_(cfg, sub_(vc, vn))); }

__device__ __forceinline__ float4 load_v(const float* v2, int i, int n, int cfg_on, float cfg) {
    float4 v = *reinterpret_cast<const float4*>(v2 + i);
    if (cfg_on) {
        const float4 u = *reinterpret_cast<const float4*>(v2 + n + i);
        v.x = cfg_blend(v.x, u.x, cfg); v.y = cfg_blend(v.y, u.y, cfg);
        v.z = cfg_blend(v.z, u.z, cfg); v.w = cfg_blend(v.w, u.w, cfg);
    }
    return v;
}

// one block
__global__ void __launch_bounds__(256) ode_time_kernel(int* step, const float* ts, float t_scale, int rk4, float* sc, float* tvec,
                                                       int rows) {
    const int i = *step;
    const float t = ts[i];
    __syncthreads();   // everyone has read the counter before it moves
    if (threadIdx.x == 0) {
        sc[0] = t;
        sc[1] = rk4 ? sub_(ts[i + 1], t) : 0.f;   // dt = ts[i+1] - ts[i], sampling.py:117
        *step = i + 1;
    }
    const float tv = mul_(t, t_scale);            // t_vec * t_scale, sampling.py:60-63
    for (int r = threadIdx.x; r < rows; r += 256) tvec[r] = tv;
}

__global__ void __launch_bounds__(256) ode_euler_update_kernel(float* x, const float* v2, int n, int cfg_on, float cfg, float dt) {
    for (int i = 4 * (blockIdx.x * 256 + threadIdx.x); i < n; i += 4 * gridDim.x * 256) {
        const float4 v = load_v(v2, i, n, cfg_on, cfg);
        float4 xv = *reinterpret_cast<float4*>(x + i);
        xv.x = add_(xv.x, mul_(v.x, dt)); xv.y = add_(xv.y, mul_(v.y, dt));    // x + pred * dt
        xv.z = add_(xv.z, mul_(v.z, dt)); xv.w = add_(xv.w, mul_(v.w, dt));
        *reinterpret_cast<float4*>(x + i) = xv;
    }
}

// time of stage `sel` of the interval in flight, with the operations that publish it to the U-Net: t | t + dt/2 | t + dt
__device__ __forceinline__ float stage_t(float t, float dt, int sel) { return sel == 0 ? t : (sel == 1 ? add_(t, dt * 0.5f) : add_(t, dt)); }
// the scaled time a kernel that closes stage 1..3 publishes for the next evaluation: tsel is 1 or 2, never t itself (the launch
// wrappers check it), so the kernels carry no arm for it
__device__ __forceinline__ float next_stage_tv(float t, float dt, int tsel, float t_scale) {
    __builtin_assume(tsel != 0);
    return mul_(stage_t(t, dt, tsel), t_scale);
}

// The state arithmetic of rk4_step, written once for every kernel that closes a stage or an interval (plain, guided, likelihood).
// the next evaluation's input: y + dt*k (full, after k3) | y + dt*k/2
__device__ __forceinline__ float4 rk4_stage_state(const float4 yv, const float4 k, float dt, int full) {
    float4 o;
    if (full) {
        o.x = add_(yv.x, mul_(dt, k.x)); o.y = add_(yv.y, mul_(dt, k.y));
        o.z = add_(yv.z, mul_(dt, k.z)); o.w = add_(yv.w, mul_(dt, k.w));
    } else {
        o.x = add_(yv.x, mul_(dt, k.x) * 0.5f); o.y = add_(yv.y, mul_(dt, k.y) * 0.5f);
        o.z = add_(yv.z, mul_(dt, k.z) * 0.5f); o.w = add_(yv.w, mul_(dt, k.w) * 0.5f);
    }
    return o;
}
__device__ __forceinline__ float rk4_comb(float y, float k1, float k2, float k3, float k4, float dt6) {
    // y + (dt/6)*(k1 + 2*k2 + 2*k3 + k4), left to right
    const float s = add_(add_(add_(k1, 2.0f * k2), 2.0f * k3), k4);
    return add_(y, mul_(dt6, s));
}
__device__ __forceinline__ float4 rk4_comb4(const float4 yv, const float4 a, const float4 b, const float4 c, const float4 k4, float dt6) {
    return make_float4(rk4_comb(yv.x, a.x, b.x, c.x, k4.x, dt6), rk4_comb(yv.y, a.y, b.y, c.y, k4.y, dt6),
                       rk4_comb(yv.z, a.z, b.z, c.z, k4.z, dt6), rk4_comb(yv.w, a.w, b.w, c.w, k4.w, dt6));
}

// Scaled time of EVERY evaluation of an integration, with the very operations the per-step kernels above use (so a conditioning table
// built from it is bit-identical to what the per-forward launches would compute): Euler: ts[i] * t_scale; RK4, interval i:
// t, t + dt/2, t + dt/2, t + dt with dt = ts[i+1] - ts[i]; rk4 == 2 (stochastic Heun), interval i: ts[i], ts[i+1].  The Euler-Maruyama
// step evaluates at ts[i] alone: the Euler pattern over its n_points - 1 intervals.
__global__ void __launch_bounds__(256) ode_all_times_kernel(const float* ts, int n_steps, int rk4, float t_scale, float* tv) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_steps) return;
    const float t = ts[i];
    if (!rk4) { tv[i] = mul_(t, t_scale); return; }
    if (rk4 == 2) {   // the stochastic Heun step: t_i, t_{i+1}, both read from the grid (ode_sde_update_kernel publishes the same product)
        tv[2 * i] = mul_(t, t_scale);
        tv[2 * i + 1] = mul_(ts[i + 1], t_scale);
        return;
    }
    const float dt = sub_(ts[i + 1], t);
    const float th = mul_(add_(t, dt * 0.5f), t_scale);
    tv[4 * i] = mul_(t, t_scale);
    tv[4 * i + 1] = th;
    tv[4 * i + 2] = th;
    tv[4 * i + 3] = mul_(add_(t, dt), t_scale);
}
int ode_all_times_launch(const float* ts, int n_steps, int rk4, float t_scale, float* tv, hipStream_t s) {
    hipLaunchKernelGGL(ode_all_times_kernel, dim3(cdiv(n_steps, 256)), dim3(256), 0, s, ts, n_steps, rk4, t_scale, tv);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

static int egrid(int n) { int g = (n / 4 + 255) / 256; return g < 1 ? 1 : (g > 2048 ? 2048 : g); }

int ode_time_launch(int* step, const float* ts, float t_scale, int rk4, float* sc, float* tvec, int rows, hipStream_t s) {
    hipLaunchKernelGGL(ode_time_kernel, dim3(1), dim3(256), 0, s, step, ts, t_scale, rk4, sc, tvec, rows);
    FC_HIP(hipGetLastError());
    return FC_OK;
}
int ode_euler_update_launch(float* x, const float* v2, int n, int cfg_on, float cfg, float dt, hipStream_t s) {
    if (n & 3) return fail(FC_E_SHAPE, "ode: element count must be a multiple of 4");
    hipLaunchKernelGGL(ode_euler_update_kernel, dim3(egrid(n)), dim3(256), 0, s, x, v2, n, cfg_on, cfg, dt);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

// ================================================================================================ measurement guidance on the RK4 grid
// fc_unet_integrate_guided: the RK4 step above with every stage velocity corrected towards a measurement ym = keep (.) x1 (the
// reference's inpainting.py algorithm3 for a diagonal operator on the conditional-OT path).  With t the time of
// the stage that produced v and x that stage's input state:
//     x1 = x + (1-t) v      w = keep (ym - keep x1) / (r2 keep^2 + s2)   (0 where the denominator is 0)      r2 = (1-t)^2 / (t^2 + (1-t)^2)
//     g  = w                      (identity)          g = w + (1-t) q,  q = (dv/dx)^T w      (exact)
//     vc = v + c g                c = gamma (1-t) / t
// The scalars om = 1-t, r2, c are formed in fp64 from the fp32 stage time and gamma and rounded once to fp32; s2 = sigma_y^2 is formed
// the same way on the host.  The elementwise part is eleven single-rounded fp32 operations in the order written in guide_w /
// guide_apply.  A correction term that is zero (gamma = 0, t = 1, keep = 0) leaves v's bits alone.
struct GuideScalars { float om, r2, c, s2; };

__device__ __forceinline__ GuideScalars guide_scalars(float t, float s2, float gamma) {
    const double td = (double)t, om = 1.0 - td;
    GuideScalars g;
    g.om = (float)om;
    g.r2 = (float)((om * om) / (td * td + om * om));
    g.c = (float)(((double)gamma * om) / td);
    g.s2 = s2;
    return g;
}
__device__ __forceinline__ float guide_w(float v, float x, float ym, float a, const GuideScalars& g) {
    const float x1 = add_(x, mul_(g.om, v));
    const float res = sub_(ym, mul_(a, x1));
    const float den = add_(mul_(g.r2, mul_(a, a)), g.s2);
    return den == 0.f ? 0.f : __fdiv_rn(mul_(a, res), den);
}
__device__ __forceinline__ float guide_apply(float v, float g, const GuideScalars& gs) {
    const float d = mul_(gs.c, g);
    return d == 0.f ? v : add_(v, d);
}
__device__ __forceinline__ float4 guide_w4(const float4 v, const float4 x, const float4 ym, const float4 a, const GuideScalars& g) {
    return make_float4(guide_w(v.x, x.x, ym.x, a.x, g), guide_w(v.y, x.y, ym.y, a.y, g), guide_w(v.z, x.z, ym.z, a.z, g),
                       guide_w(v.w, x.w, ym.w, a.w, g));
}
// v corrected at element i; q == nullptr: identity form
__device__ __forceinline__ float4 guide_v4(const float4 v, const float* xin, const float* ym, const float* keep, const float* q, int i,
                                           const GuideScalars& g) {
    float4 w = guide_w4(v, *reinterpret_cast<const float4*>(xin + i), *reinterpret_cast<const float4*>(ym + i),
                        *reinterpret_cast<const float4*>(keep + i), g);
    if (q) {
        const float4 qv = *reinterpret_cast<const float4*>(q + i);
        w.x = add_(w.x, mul_(g.om, qv.x)); w.y = add_(w.y, mul_(g.om, qv.y));
        w.z = add_(w.z, mul_(g.om, qv.z)); w.w = add_(w.w, mul_(g.om, qv.w));
    }
    return make_float4(guide_apply(v.x, w.x, g), guide_apply(v.y, w.y, g), guide_apply(v.z, w.z, g), guide_apply(v.w, w.w, g));
}

// One stage of rk4_step closed: k_out = the evaluation's velocity, xs = the next evaluation's input, tvec = its time (stage `tsel`).
// Guided: the correction sits between load_v and the store of k; g.xin is the state this stage's forward read (y for k1, xs for k2 and
// k3; xs[i] is read before this thread overwrites it), g.tcur that stage's time.  The plain instantiation holds no guidance code.
template <bool Guided>
__global__ void __launch_bounds__(256) ode_rk4_stage_kernel(const float* sc, const float* y, float* xs, float* k_out, const float* v2,
                                                            int n, int cfg_on, float cfg, int full, int tsel, float t_scale,
                                                            float* tvec, int rows, Rk4Guide g) {
    const float t = sc[0], dt = sc[1];
    if (blockIdx.x == 0) {
        const float tv = next_stage_tv(t, dt, tsel, t_scale);
        for (int r = threadIdx.x; r < rows; r += 256) tvec[r] = tv;
    }
    GuideScalars gs{};
    if constexpr (Guided) gs = guide_scalars(stage_t(t, dt, g.tcur), g.gsc[0], g.gsc[1]);
    for (int i = 4 * (blockIdx.x * 256 + threadIdx.x); i < n; i += 4 * gridDim.x * 256) {
        float4 k = load_v(v2, i, n, cfg_on, cfg);
        if constexpr (Guided) k = guide_v4(k, g.xin, g.ym, g.keep, g.q, i, gs);
        *reinterpret_cast<float4*>(k_out + i) = k;
        *reinterpret_cast<float4*>(xs + i) = rk4_stage_state(*reinterpret_cast<const float4*>(y + i), k, dt, full);
    }
}

// The interval closed: y += (dt/6)(k1 + 2 k2 + 2 k3 + k4).  Guided: k4 corrected at (g.xin = xs, t + dt)
template <bool Guided>
__global__ void __launch_bounds__(256) ode_rk4_final_kernel(const float* sc, float* y, const float* k1, const float* k2, const float* k3,
                                                            const float* v2, int n, int cfg_on, float cfg, Rk4Guide g) {
    const float dt6 = __fdiv_rn(sc[1], 6.0f);
    GuideScalars gs{};
    if constexpr (Guided) gs = guide_scalars(stage_t(sc[0], sc[1], 2), g.gsc[0], g.gsc[1]);
    for (int i = 4 * (blockIdx.x * 256 + threadIdx.x); i < n; i += 4 * gridDim.x * 256) {
        float4 k4 = load_v(v2, i, n, cfg_on, cfg);
        if constexpr (Guided) k4 = guide_v4(k4, g.xin, g.ym, g.keep, g.q, i, gs);
        const float4 a = *reinterpret_cast<const float4*>(k1 + i), b = *reinterpret_cast<const float4*>(k2 + i),
                     c = *reinterpret_cast<const float4*>(k3 + i);
        *reinterpret_cast<float4*>(y + i) = rk4_comb4(*reinterpret_cast<float4*>(y + i), a, b, c, k4, dt6);
    }
}

// exact mode: w of the running stage, the cotangent the data-gradient chain takes (no guidance pair: v is the forward's output)
__global__ void __launch_bounds__(256) ode_guide_w_kernel(const float* sc, const float* gsc, const float* v, const float* xin,
                                                          const float* ym, const float* keep, float* w, int n, int tcur) {
    const GuideScalars g = guide_scalars(stage_t(sc[0], sc[1], tcur), gsc[0], gsc[1]);
    for (int i = 4 * (blockIdx.x * 256 + threadIdx.x); i < n; i += 4 * gridDim.x * 256)
        *reinterpret_cast<float4*>(w + i) = guide_w4(*reinterpret_cast<const float4*>(v + i), *reinterpret_cast<const float4*>(xin + i),
                                                     *reinterpret_cast<const float4*>(ym + i), *reinterpret_cast<const float4*>(keep + i), g);
}

// fc_ode_guided_correct: the identity-form correction of one evaluation on caller tensors
__global__ void __launch_bounds__(256) ode_guided_correct_kernel(const float* v, const float* x, const float* ym, const float* keep,
                                                                 float* out, int n, float t, float s2, float gamma) {
    const GuideScalars g = guide_scalars(t, s2, gamma);
    for (int i = 4 * (blockIdx.x * 256 + threadIdx.x); i < n; i += 4 * gridDim.x * 256)
        *reinterpret_cast<float4*>(out + i) = guide_v4(*reinterpret_cast<const float4*>(v + i), x, ym, keep, nullptr, i, g);
}

int ode_rk4_stage_launch(const float* sc, const float* y, float* xs, float* k_out, const float* v2, int n, int cfg_on, float cfg, int full,
                         int tsel, float t_scale, float* tvec, int rows, const Rk4Guide* g, hipStream_t s) {
    if (n & 3) return fail(FC_E_SHAPE, "ode: element count must be a multiple of 4");
    if (g && (g->tcur < 0 || g->tcur > 2)) return fail(FC_E_ARG, "ode: stage time selector must lie in [0, 2]");
    if (tsel < 1 || tsel > 2) return fail(FC_E_ARG, "ode: the next stage's time selector must lie in [1, 2]");
    hipLaunchKernelGGL(g ? ode_rk4_stage_kernel<true> : ode_rk4_stage_kernel<false>, dim3(egrid(n)), dim3(256), 0, s, sc, y, xs, k_out, v2,
                       n, cfg_on, cfg, full, tsel, t_scale, tvec, rows, g ? *g : Rk4Guide{});
    FC_HIP(hipGetLastError());
    return FC_OK;
}
int ode_rk4_final_launch(const float* sc, float* y, const float* k1, const float* k2, const float* k3, const float* v2, int n, int cfg_on,
                         float cfg, const Rk4Guide* g, hipStream_t s) {
    if (n & 3) return fail(FC_E_SHAPE, "ode: element count must be a multiple of 4");
    hipLaunchKernelGGL(g ? ode_rk4_final_kernel<true> : ode_rk4_final_kernel<false>, dim3(egrid(n)), dim3(256), 0, s, sc, y, k1, k2, k3, v2,
                       n, cfg_on, cfg, g ? *g : Rk4Guide{});
    FC_HIP(hipGetLastError());
    return FC_OK;
}
int ode_guide_w_launch(const float* sc, const float* gsc, const float* v, const float* xin, const float* ym, const float* keep, float* w,
                       int n, int tcur, hipStream_t s) {
    if (n & 3) return fail(FC_E_SHAPE, "ode: element count must be a multiple of 4");
    if (tcur < 0 || tcur > 2) return fail(FC_E_ARG, "ode: stage time selector must lie in [0, 2]");
    hipLaunchKernelGGL(ode_guide_w_kernel, dim3(egrid(n)), dim3(256), 0, s, sc, gsc, v, xin, ym, keep, w, n, tcur);
    FC_HIP(hipGetLastError());
    return FC_OK;
}
int ode_guided_correct_launch(const float* v, const float* x, const float* ym, const float* keep, float* out, int n, float t, float s2,
                              float gamma, hipStream_t s) {
    if (n < 4 || (n & 3)) return fail(FC_E_SHAPE, "ode: element count must be a positive multiple of 4");
    hipLaunchKernelGGL(ode_guided_correct_kernel, dim3(egrid(n)), dim3(256), 0, s, v, x, ym, keep, out, n, t, s2, gamma);
    FC_HIP(hipGetLastError());
    return FC_OK;
}


// ================================================================================================ adaptive RK45
// scipy.integrate.solve_ivp(method="RK45") as the legacy sampler calls it (legacy/train_sd_flowers.py:78-107): scipy 1.15's
// _ivp/rk.py (rk_step, RungeKutta._step_impl, RK45 tableau) and _ivp/common.py (select_initial_step, norm).  y, y_new, the stage sums,
// the scale and the error are fp64; every forward gets float32(y_stage) and time float32(t + c h) * t_scale (fp32); the stage
// derivatives K_i are the fp32 forwards (scipy's fp64 copies of them are exact).  Controller decisions happen on the device
// (Rk45State); the host only reads the status summary behind each attempt.
//
// Controller groups (Rk45Groups): st[g] is one solve_ivp problem over the m unknowns of rows g*spg .. g*spg + spg - 1 (with CFG also
// their unguided twins B + row, B = G*spg), with its own select_initial_step, error norm, step size, accept / reject decisions and
// counters.  The batch-coupled sampler is ONE group of all B rows, as the legacy sampler (one step size and one error norm for the
// whole batch); the per-sample sampler is one group per sample.  The elementwise and partial-sum kernels run on a (chunks, G) grid:
// blockIdx.y is the group, and its `chunks` workgroups stride over its m unknowns; one workgroup per group reduces the fp64 partial
// sums ([G][chunks][2]) in a fixed order.  `chunks` fixes the summation order and with it the bits of the norms (the host picks it).
// A group that has finished or failed keeps h = 0: its rows are still evaluated (at float32(y), t), its state, counters and K stay
// as they are.
//
// Dense output (solve_ivp's t_eval, Rk45Eval): the step sequence is untouched.  The controller of an accepted step records which
// requested times fall into it, and rk45_dense -- between the decision and the commit, while y and K0..K6 of the step still stand --
// writes the step's quartic interpolant (RkDenseOutput) at those times into the caller's frames.
//
// The likelihood's augmented state (fc_unet_log_likelihood_rk45, Rk45LL): a group's solve_ivp vector is y = [x (m), a (spg)] with
// da[r]/dt = d[r] = sum eps g of row r, so n = m + spg unknowns enter every norm.  f does not read a, hence the stage states of the
// a-component feed nothing and the x kernels are the sampler's as they stand; the a-component's seven K values are the fp64 row sums
// ll.d[s][r] (ode_ll_dot_kernel behind every evaluation), and everything the a-component adds -- its terms of select_initial_step's
// three norms, a_new = a + h sum B_s d_s, its term of the error norm with scale atol + rtol max(|a|, |a_new|), the commit a <- a_new,
// d_0 <- d_6 -- is done by the one thread that owns the group's controller, after the x partials, one term per row in row order.
// LL is a template flag of those three kernels: the sampler's instantiations hold none of it.

__constant__ double c_rk45_C[7] = {0.0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 1.0};
__constant__ double c_rk45_A[6][5] = {
    {0, 0, 0, 0, 0},
    {1.0 / 5, 0, 0, 0, 0},
    {3.0 / 40, 9.0 / 40, 0, 0, 0},
    {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0},
    {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0},
    {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656}};
__constant__ double c_rk45_B[6] = {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84};
__constant__ double c_rk45_E[7] = {-71.0 / 57600, 0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200, -22.0 / 525, 1.0 / 40};

// Python's min(a, b) / max(a, b) (first argument unless the second compares smaller / larger: NaN handling as scipy sees it)
__device__ __forceinline__ double py_min(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double py_max(double a, double b) { return b > a ? b : a; }
// np.maximum: NaN propagates
__device__ __forceinline__ double np_maximum(double a, double b) { return (a != a || b != b) ? a + b : (a > b ? a : b); }

// sum of a block's 256 per-thread values, fixed tree order; valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

// one workgroup: total of `nblk` partial sums (stride `stride`, offset `off`) in a fixed order
__device__ __forceinline__ double reduce_parts(const double* part, int nblk, int stride, int off, double* red) {
    double v = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) v += part[(size_t)b * stride + off];
    const double r = block_sum(v, red);
    __syncthreads();
    return r;
}

__device__ __forceinline__ float stage_time(double t, float t_scale) { return mul_((float)t, t_scale); }   // ones(B) * t * 999

// the time rows of group g (every thread of one workgroup): its spg rows and, with CFG, their unguided twins G*spg + row
__device__ __forceinline__ void write_trows(float* tvec, int g, int G, int spg, int cfg_on, float tv) {
    for (int r = g * spg + threadIdx.x; r < (g + 1) * spg; r += 256) {
        tvec[r] = tv;
        if (cfg_on) tvec[G * spg + r] = tv;
    }
}

__device__ __forceinline__ bool rk45_live(const Rk45State& s) { return !s.done && !s.failed; }

// after a decision: a finished or failed group keeps h = 0
__device__ __forceinline__ void rk45_freeze(Rk45State* st) {
    if (!rk45_live(*st)) { st->h = 0.0; st->t_new = st->t; }
}

// this workgroup's pair of partial sums in the [G][chunks][2] buffer
__device__ __forceinline__ double* group_part(double* part, int g) { return part + 2 * ((size_t)g * gridDim.x + blockIdx.x); }

// RungeKutta._step_impl up to rk_step: the h and t_new of the next attempt.  `start`: a new step (after select_initial_step or an
// acceptance) -- h_abs is raised to min_step there; after a rejection it is not, and h_abs < min_step fails.
__device__ void rk45_next_attempt(Rk45State* st, bool start) {
    const double t = st->t, dir = st->dir;
    const double min_step = 10.0 * fabs(nextafter(t, dir * (double)INFINITY) - t);
    double h_abs = st->h_abs;
    if (start && h_abs < min_step) h_abs = min_step;     // (max_step is inf)
    if (h_abs < min_step) { st->failed = 1; return; }
    if (st->attempts >= st->max_attempts) { st->failed = 2; return; }
    double h = h_abs * dir;
    double t_new = t + h;
    if (dir * (t_new - st->t_bound) > 0) t_new = st->t_bound;
    h = t_new - t;
    st->h = h; st->t_new = t_new; st->h_abs = fabs(h);
}

__device__ __forceinline__ void load_y4(const double* y, int i, double o[4]) {
    const double2 a = *reinterpret_cast<const double2*>(y + i), b = *reinterpret_cast<const double2*>(y + i + 2);
    o[0] = a.x; o[1] = a.y; o[2] = b.x; o[3] = b.y;
}
__device__ __forceinline__ void f4_to(const float4 v, double o[4]) { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }

// xs = float32(y) over this workgroup's part of a group (the rows of a group that no longer steps)
__device__ __forceinline__ void rk45_hold(const double* y, float* xs, int base, int m) {
    for (int j = 4 * (blockIdx.x * 256 + threadIdx.x); j < m; j += 4 * gridDim.x * 256) {
        double yv[4];
        load_y4(y, base + j, yv);
        *reinterpret_cast<float4*>(xs + base + j) = make_float4((float)yv[0], (float)yv[1], (float)yv[2], (float)yv[3]);
    }
}

// y = double(x), xs = x (the first forward's input), controller state, time rows of f(t0, y0)
__global__ void __launch_bounds__(256) rk45_setup_kernel(const float* x, double* y, float* xs, int m, int spg, Rk45State* st, double t0,
                                                         double t1, double rtol, double atol, int max_attempts, float t_scale, float* tvec,
                                                         int cfg_on) {
    const int g = blockIdx.y, base = g * m;
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) {
            Rk45State s{};
            s.t = t0; s.t_bound = t1; s.dir = t1 > t0 ? 1.0 : -1.0; s.rtol = rtol; s.atol = atol; s.max_attempts = max_attempts;
            s.nfev = 1;
            st[g] = s;
        }
        write_trows(tvec, g, gridDim.y, spg, cfg_on, stage_time(t0, t_scale));
    }
    for (int j = 4 * (blockIdx.x * 256 + threadIdx.x); j < m; j += 4 * gridDim.x * 256) {
        const float4 v = *reinterpret_cast<const float4*>(x + base + j);
        *reinterpret_cast<float4*>(xs + base + j) = v;
        *reinterpret_cast<double2*>(y + base + j) = make_double2(v.x, v.y);
        *reinterpret_cast<double2*>(y + base + j + 2) = make_double2(v.z, v.w);
    }
}

// select_initial_step, part 1: f0 = blend(v2) -> K0; partial sums of (y0/scale)^2 and (f0/scale)^2, scale = atol + |y0| rtol
__global__ void __launch_bounds__(256) rk45_d01_kernel(const Rk45State* st, const double* y, float* k0, const float* v2, int m,
                                                       int cfg_on, float cfg, double* part) {
    __shared__ double red[256];
    const int g = blockIdx.y, base = g * m, n = gridDim.y * m;
    const double rtol = st[g].rtol, atol = st[g].atol;
    double s0 = 0.0, s1 = 0.0;
    for (int j = 4 * (blockIdx.x * 256 + threadIdx.x); j < m; j += 4 * gridDim.x * 256) {
        const int i = base + j;
        const float4 f = load_v(v2, i, n, cfg_on, cfg);
        *reinterpret_cast<float4*>(k0 + i) = f;
        double yv[4], fv[4];
        load_y4(y, i, yv); f4_to(f, fv);
        for (int q = 0; q < 4; ++q) {
            const double sc = atol + fabs(yv[q]) * rtol;
            const double a = yv[q] / sc, c = fv[q] / sc;
            s0 += a * a; s1 += c * c;
        }
    }
    const double r0 = block_sum(s0, red);
    __syncthreads();
    const double r1 = block_sum(s1, red);
    if (threadIdx.x == 0) { double* p = group_part(part, g); p[0] = r0; p[1] = r1; }
}

// select_initial_step up to h0, from the sums of (y0/scale)^2 and (f0/scale)^2 over n unknowns; returns h0
__device__ __forceinline__ double rk45_select_h0(Rk45State* st, double s0, double s1, int n) {
    const double rn = sqrt((double)n);
    const double d0 = sqrt(s0) / rn, d1 = sqrt(s1) / rn;
    double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    h0 = py_min(h0, fabs(st->t_bound - st->t));
    st->h0 = h0; st->d1 = d1;
    return h0;
}

// select_initial_step, part 2 (one workgroup per group): d0, d1 -> h0; time rows of f(t0 + h0 dir, y1)
template <bool LL>
__global__ void __launch_bounds__(256) rk45_h0_kernel(Rk45State* st, const double* part, int chunks, int m, int spg, float t_scale,
                                                      float* tvec, int cfg_on, Rk45LL ll) {
    __shared__ double red[256];
    const int g = blockIdx.x;
    const double* p = part + 2 * (size_t)g * chunks;
    double s0 = reduce_parts(p, chunks, 2, 0, red), s1 = reduce_parts(p, chunks, 2, 1, red);
    if (threadIdx.x == 0) {
        Rk45State* sg = st + g;
        if constexpr (LL) {   // the a-component: y0 = a, f0 = d_0
            for (int r = g * spg; r < (g + 1) * spg; ++r) {
                const double sc = sg->atol + fabs(ll.a[r]) * sg->rtol;
                const double a = ll.a[r] / sc, c = ll.d[r] / sc;
                s0 += a * a; s1 += c * c;
            }
        }
        const double h0 = rk45_select_h0(sg, s0, s1, LL ? m + spg : m);
        const float tv = stage_time(sg->t + h0 * sg->dir, t_scale);
        for (int r = g * spg; r < (g + 1) * spg; ++r) {   // (runs once per solve: one thread writes the group's rows)
            tvec[r] = tv;
            if (cfg_on) tvec[gridDim.x * spg + r] = tv;
        }
    }
}

// xs = float32(y0 + h0 dir f0)
__global__ void __launch_bounds__(256) rk45_y1_kernel(const Rk45State* st, const double* y, const float* k0, float* xs, int m) {
    const int g = blockIdx.y, base = g * m;
    const double hd = st[g].h0 * st[g].dir;
    for (int j = 4 * (blockIdx.x * 256 + threadIdx.x); j < m; j += 4 * gridDim.x * 256) {
        const int i = base + j;
        double yv[4], fv[4];
        load_y4(y, i, yv); f4_to(*reinterpret_cast<const float4*>(k0 + i), fv);
        float4 o;
        o.x = (float)(yv[0] + hd * fv[0]); o.y = (float)(yv[1] + hd * fv[1]);
        o.z = (float)(yv[2] + hd * fv[2]); o.w = (float)(yv[3] + hd * fv[3]);
        *reinterpret_cast<float4*>(xs + i) = o;
    }
}

// select_initial_step, part 3: partial sums of ((f1 - f0)/scale)^2
__global__ void __launch_bounds__(256) rk45_d2_kernel(const Rk45State* st, const double* y, const float* k0, const float* v2, int m,
                                                      int cfg_on, float cfg, double* part) {
    __shared__ double red[256];
    const int g = blockIdx.y, base = g * m, n = gridDim.y * m;
    const double rtol = st[g].rtol, atol = st[g].atol;
    double s = 0.0;
    for (int j = 4 * (blockIdx.x * 256 + threadIdx.x); j < m; j += 4 * gridDim.x * 256) {
        const int i = base + j;
        double yv[4], f0[4], f1[4];
        load_y4(y, i, yv); f4_to(*reinterpret_cast<const float4*>(k0 + i), f0); f4_to(load_v(v2, i, n, cfg_on, cfg), f1);
        for (int q = 0; q < 4; ++q) {
            const double a = (f1[q] - f0[q]) / (atol + fabs(yv[q]) * rtol);
            s += a * a;
        }
    }
    const double r = block_sum(s, red);
    if (threadIdx.x == 0) group_part(part, g)[0] = r;
}

// select_initial_step from the sum of ((f1 - f0)/scale)^2 over n unknowns: h1, the first step, the first attempt
__device__ __forceinline__ void rk45_select_h1(Rk45State* st, double s2, int n) {
    const double h0 = st->h0, d1 = st->d1;
    const double d2 = sqrt(s2) / sqrt((double)n) / h0;
    const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? py_max(1e-6, h0 * 1e-3) : pow(0.01 / py_max(d1, d2), 1.0 / (4 + 1));
    st->h_abs = py_min(py_min(100 * h0, h1), fabs(st->t_bound - st->t));
    st->nfev = 2;
    rk45_next_attempt(st, true);
}

// select_initial_step, part 4 (one workgroup per group): d2 -> h1 -> first step; the first attempt's h and t_new
template <bool LL>
__global__ void __launch_bounds__(256) rk45_h1_kernel(Rk45State* st, const double* part, int chunks, int m, int spg, Rk45LL ll) {
    __shared__ double red[256];
    const int g = blockIdx.x;
    double s2 = reduce_parts(part + 2 * (size_t)g * chunks, chunks, 2, 0, red);
    if (threadIdx.x == 0) {
        if constexpr (LL) {   // the a-component: f1 = d_1 (the evaluation at y0 + h0 f0), f0 = d_0
            for (int r = g * spg; r < (g + 1) * spg; ++r) {
                const double a = (ll.d[ll.B + r] - ll.d[r]) / (st[g].atol + fabs(ll.a[r]) * st[g].rtol);
                s2 += a * a;
            }
        }
        rk45_select_h1(st + g, s2, LL ? m + spg : m);
        rk45_freeze(st + g);
    }
}

// Stage s = 1..5 of rk_step: K[s-1] = blend(v2) (s >= 2; K0 is the committed f); xs = float32(y + (sum_{j<s} A[s][j] K_j) h);
// time rows of stage s.
template <int s>
__global__ void __launch_bounds__(256) rk45_stage_kernel(const Rk45State* st, const double* y, Rk45K kk, const float* v2, int m, int spg,
                                                         int cfg_on, float cfg, float* xs, float t_scale, float* tvec) {
    const int g = blockIdx.y, base = g * m, n = gridDim.y * m;
    const double h = st[g].h;
    if (blockIdx.x == 0) write_trows(tvec, g, gridDim.y, spg, cfg_on, stage_time(st[g].t + c_rk45_C[s] * h, t_scale));
    if (!rk45_live(st[g])) { rk45_hold(y, xs, base, m); return; }
    float* kprev = kk.k[s - 1];
    for (int jj = 4 * (blockIdx.x * 256 + threadIdx.x); jj < m; jj += 4 * gridDim.x * 256) {
        const int i = base + jj;
        double acc[4] = {0.0, 0.0, 0.0, 0.0}, kv[4];
#pragma unroll
        for (int j = 0; j < s; ++j) {
            float4 k;
            if (j == s - 1 && s >= 2) { k = load_v(v2, i, n, cfg_on, cfg); *reinterpret_cast<float4*>(kprev + i) = k; }
            else k = *reinterpret_cast<const float4*>(kk.k[j] + i);
            f4_to(k, kv);
            const double a = c_rk45_A[s][j];
            for (int q = 0; q < 4; ++q) acc[q] = j == 0 ? kv[q] * a : acc[q] + kv[q] * a;
        }
        double yv[4];
        load_y4(y, i, yv);
        float4 o;
        o.x = (float)(yv[0] + acc[0] * h); o.y = (float)(yv[1] + acc[1] * h);
        o.z = (float)(yv[2] + acc[2] * h); o.w = (float)(yv[3] + acc[3] * h);
        *reinterpret_cast<float4*>(xs + i) = o;
    }
}

// K5 = blend(v2); y_new = y + h (sum_j B_j K_j); xs = float32(y_new); time rows of f(t + h, y_new)
__global__ void __launch_bounds__(256) rk45_finish_kernel(const Rk45State* st, const double* y, double* y_new, Rk45K kk,
                                                          const float* v2, int m, int spg, int cfg_on, float cfg, float* xs,
                                                          float t_scale, float* tvec) {
    const int g = blockIdx.y, base = g * m, n = gridDim.y * m;
    const double h = st[g].h;
    if (blockIdx.x == 0) write_trows(tvec, g, gridDim.y, spg, cfg_on, stage_time(st[g].t + h, t_scale));
    if (!rk45_live(st[g])) { rk45_hold(y, xs, base, m); return; }
    for (int jj = 4 * (blockIdx.x * 256 + threadIdx.x); jj < m; jj += 4 * gridDim.x * 256) {
        const int i = base + jj;
        double acc[4], kv[4];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            float4 k;
            if (j == 5) { k = load_v(v2, i, n, cfg_on, cfg); *reinterpret_cast<float4*>(kk.k[5] + i) = k; }
            else k = *reinterpret_cast<const float4*>(kk.k[j] + i);
            f4_to(k, kv);
            const double c = c_rk45_B[j];
            for (int q = 0; q < 4; ++q) acc[q] = j == 0 ? kv[q] * c : acc[q] + kv[q] * c;
        }
        double yv[4], o[4];
        load_y4(y, i, yv);
        for (int q = 0; q < 4; ++q) o[q] = yv[q] + h * acc[q];
        *reinterpret_cast<double2*>(y_new + i) = make_double2(o[0], o[1]);
        *reinterpret_cast<double2*>(y_new + i + 2) = make_double2(o[2], o[3]);
        *reinterpret_cast<float4*>(xs + i) = make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]);
    }
}

// K6 = blend(v2) = f(t + h, y_new); partial sums of ((sum_j E_j K_j) h / scale)^2, scale = atol + max(|y|, |y_new|) rtol
__global__ void __launch_bounds__(256) rk45_error_kernel(const Rk45State* st, const double* y, const double* y_new, Rk45K kk,
                                                         const float* v2, int m, int cfg_on, float cfg, double* part) {
    __shared__ double red[256];
    const int g = blockIdx.y, base = g * m, n = gridDim.y * m;
    const double h = st[g].h, rtol = st[g].rtol, atol = st[g].atol;
    double s = 0.0;
    if (rk45_live(st[g])) {
        for (int jj = 4 * (blockIdx.x * 256 + threadIdx.x); jj < m; jj += 4 * gridDim.x * 256) {
            const int i = base + jj;
            double acc[4], kv[4];
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                float4 k;
                if (j == 6) { k = load_v(v2, i, n, cfg_on, cfg); *reinterpret_cast<float4*>(kk.k[6] + i) = k; }
                else k = *reinterpret_cast<const float4*>(kk.k[j] + i);
                f4_to(k, kv);
                const double e = c_rk45_E[j];
                for (int q = 0; q < 4; ++q) acc[q] = j == 0 ? kv[q] * e : acc[q] + kv[q] * e;
            }
            double yv[4], yn[4];
            load_y4(y, i, yv); load_y4(y_new, i, yn);
            for (int q = 0; q < 4; ++q) {
                const double sc = atol + np_maximum(fabs(yv[q]), fabs(yn[q])) * rtol;
                const double a = acc[q] * h / sc;
                s += a * a;
            }
        }
    }
    const double r = block_sum(s, red);
    if (threadIdx.x == 0) group_part(part, g)[0] = r;
}

// solve_ivp's t_eval bookkeeping behind an accepted step that ended at st->t: the not-yet-served requested times with
// dir (te - t) <= 0 ("the value in t_eval equal to t will be included": searchsorted side='right', 'left' on the reversed array when
// integrating backwards).  Only this thread moves the cursor; rk45_dense reads the finished record in the next launch.
__device__ __forceinline__ void rk45_eval_range(Rk45State* st, const Rk45Eval* ev) {
    const double* te = rk45_eval_times(ev);
    const int n_eval = ev->n_eval;
    int end = st->ev_cursor;
    st->ev_first = end;
    while (end < n_eval && st->dir * (te[end] - st->t) <= 0) ++end;
    st->ev_end = st->ev_cursor = end;
}

// Accept / reject on the error norm `en` (RungeKutta._step_impl), the next attempt, the status record
__device__ __forceinline__ void rk45_decide(Rk45State* st, double en) {
    const double expo = -1.0 / (4 + 1);
    st->err = en;
    st->nfev += 6;
    st->attempts += 1;
    double h_abs = st->h_abs;
    if (en < 1) {
        double factor = en == 0 ? 10.0 : py_min(10.0, 0.9 * pow(en, expo));
        if (st->step_rejected) factor = py_min(1.0, factor);
        st->h_abs = h_abs * factor;
        st->t_old = st->t;
        st->t = st->t_new;
        st->accepted += 1;
        st->accepted_last = 1;
        st->step_rejected = 0;
        if (st->dir * (st->t - st->t_bound) >= 0) { st->done = 1; return; }
        rk45_next_attempt(st, true);
    } else {
        st->h_abs = h_abs * py_max(0.2, 0.9 * pow(en, expo));
        st->rejected += 1;
        st->accepted_last = 0;
        st->step_rejected = 1;
        rk45_next_attempt(st, false);
    }
}

// h sum_s B_s K_s over the seven K values k[s * stride] of one a-component (rk_step's sum, left to right as the x kernels'): the one
// expression behind a_new of the mean row and behind every probe's own integral
__device__ __forceinline__ double rk45_ll_bsum(const double* k, size_t stride) {
    double yn = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) yn = j == 0 ? k[0] * c_rk45_B[j] : yn + k[(size_t)j * stride] * c_rk45_B[j];
    return yn;
}
__device__ __forceinline__ double rk45_ll_advance(double a, double h, double yn) { return a + h * yn; }

// The a-component of row r in the attempt just evaluated (rk_step and the error estimate on ll.d[0..6][r], sums left to right as the x
// kernels'): a_new into ll.a[B + r]; returns its term of the error norm's sum
__device__ __forceinline__ double rk45_ll_row(const Rk45State& sg, const Rk45LL& ll, int r) {
    double er = 0.0;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const double k = ll.d[(size_t)j * ll.B + r];
        er = j == 0 ? k * c_rk45_E[j] : er + k * c_rk45_E[j];
    }
    const double a = ll.a[r], a_new = rk45_ll_advance(a, sg.h, rk45_ll_bsum(ll.d + r, ll.B));
    ll.a[ll.B + r] = a_new;
    const double e = er * sg.h / (sg.atol + np_maximum(fabs(a), fabs(a_new)) * sg.rtol);
    return e * e;
}

// Row r's commit of an accepted step of size h: a <- a_new, d_0 <- d_6 (FSAL), and with per-probe rows (ll.dk) each probe's own
// integral a_k <- a_k + h sum_s B_s d_{s,k} -- a by-product outside the norm, formed as a_new is -- and its d_{0,k} <- d_{6,k}.
__device__ __forceinline__ void rk45_ll_commit(const Rk45LL& ll, int r, double h) {
    ll.a[r] = ll.a[ll.B + r];
    ll.d[r] = ll.d[(size_t)6 * ll.B + r];
    const size_t KB = (size_t)ll.K * ll.B;
    for (int k = 0; k < ll.K && ll.dk; ++k) {
        double* dk = ll.dk + (size_t)k * ll.B + r;
        ll.ak[(size_t)k * ll.B + r] = rk45_ll_advance(ll.ak[(size_t)k * ll.B + r], h, rk45_ll_bsum(dk, KB));
        dk[0] = dk[6 * KB];
    }
}

// one workgroup per group: its error norm and decision, and with a dense-output request (`ev`) the requested times an accepted step
// serves; a group that no longer steps only clears accepted_last.  LL: the rows' a-components join the norm, and an accepted step
// commits them here (a <- a_new, d_0 <- d_6: FSAL), where the thread that owns them is
template <bool LL>
__global__ void __launch_bounds__(256) rk45_control_kernel(Rk45State* st, const double* part, int chunks, int m, int spg, const Rk45Eval* ev,
                                                           Rk45LL ll) {
    __shared__ double red[256];
    const int g = blockIdx.x;
    Rk45State* sg = st + g;
    if (!rk45_live(*sg)) {
        if (threadIdx.x == 0) sg->accepted_last = 0;
        return;
    }
    double s = reduce_parts(part + 2 * (size_t)g * chunks, chunks, 2, 0, red);
    if (threadIdx.x != 0) return;
    const double h = sg->h;   // the attempt's step (rk45_decide writes the next attempt's)
    if constexpr (LL)
        for (int r = g * spg; r < (g + 1) * spg; ++r) s += rk45_ll_row(*sg, ll, r);
    rk45_decide(sg, sqrt(s) / sqrt((double)(LL ? m + spg : m)));
    if constexpr (LL) {
        if (sg->accepted_last)
            for (int r = g * spg; r < (g + 1) * spg; ++r) rk45_ll_commit(ll, r, h);
    }
    if (ev && sg->accepted_last) rk45_eval_range(sg, ev);
    rk45_freeze(sg);
}

// scipy's RK45.P: the quartic interpolant of a step is y_old + h (Q p), Q = K^T P, p = (x, x^2, x^3, x^4), x = (t - t_old) / h
__constant__ double c_rk45_P[7][4] = {
    {1, -8048581381.0 / 2820520608, 8663915743.0 / 2820520608, -12715105075.0 / 11282082432},
    {0, 0, 0, 0},
    {0, 131558114200.0 / 32700410799, -68118460800.0 / 10900136933, 87487479700.0 / 32700410799},
    {0, -1754552775.0 / 470086768, 14199869525.0 / 1410260304, -10690763975.0 / 1880347072},
    {0, 127303824393.0 / 49829197408, -318862633887.0 / 49829197408, 701980252875.0 / 199316789632},
    {0, -282668133.0 / 205662961, 2019193451.0 / 616988883, -1453857185.0 / 822651844},
    {0, 40617522.0 / 29380423, -110615467.0 / 29380423, 69997945.0 / 29380423}};

// Dense output of the step just accepted (RkDenseOutput._call_impl), before the commit overwrites y and K0: for every requested time
// j in the range the controller recorded, frames[j] = float32(y + h (Q p_j)) over this group's unknowns.  All fp64 with the fp32 K_s
// widened exactly, sums left to right; Q is formed once per element and serves every j of the step.  Elementwise: the bits do not
// depend on `chunks`.  (Row 1 of P is zero; K1 is read all the same so that a non-finite K1 spreads as it does in scipy.)
__global__ void __launch_bounds__(256) rk45_dense_kernel(const Rk45State* st, const Rk45Eval* ev, const double* y, Rk45K kk, int m) {
    const int g = blockIdx.y, base = g * m;
    if (!st[g].accepted_last) return;
    const int first = st[g].ev_first, end = st[g].ev_end;
    if (first >= end) return;
    const double t_old = st[g].t_old, h = st[g].t - t_old;
    const double* te = rk45_eval_times(ev);
    float* frames = ev->frames;
    const size_t n = (size_t)gridDim.y * m;
    for (int jj = 4 * (blockIdx.x * 256 + threadIdx.x); jj < m; jj += 4 * gridDim.x * 256) {
        const int i = base + jj;
        double q[4][4], kv[4];
#pragma unroll
        for (int s = 0; s < 7; ++s) {
            f4_to(*reinterpret_cast<const float4*>(kk.k[s] + i), kv);
            for (int c = 0; c < 4; ++c) {
                const double pc = c_rk45_P[s][c];
                for (int l = 0; l < 4; ++l) q[c][l] = s == 0 ? kv[l] * pc : q[c][l] + kv[l] * pc;
            }
        }
        double yv[4];
        load_y4(y, i, yv);
        for (int j = first; j < end; ++j) {
            const double x = (te[j] - t_old) / h;
            const double p1 = x * x, p2 = p1 * x, p3 = p2 * x;          // cumprod([x, x, x, x])
            double o[4];
            for (int l = 0; l < 4; ++l) o[l] = yv[l] + h * (q[0][l] * x + q[1][l] * p1 + q[2][l] * p2 + q[3][l] * p3);
            *reinterpret_cast<float4*>(frames + (size_t)j * n + i) = make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]);
        }
    }
}

// on acceptance: y <- y_new, K0 <- K6 (FSAL)
__global__ void __launch_bounds__(256) rk45_commit_kernel(const Rk45State* st, double* y, const double* y_new, float* k0, const float* k6,
                                                          int m) {
    const int g = blockIdx.y, base = g * m;
    if (!st[g].accepted_last) return;
    for (int jj = 4 * (blockIdx.x * 256 + threadIdx.x); jj < m; jj += 4 * gridDim.x * 256) {
        const int i = base + jj;
        *reinterpret_cast<double2*>(y + i) = *reinterpret_cast<const double2*>(y_new + i);
        *reinterpret_cast<double2*>(y + i + 2) = *reinterpret_cast<const double2*>(y_new + i + 2);
        *reinterpret_cast<float4*>(k0 + i) = *reinterpret_cast<const float4*>(k6 + i);
    }
}

// one workgroup: how many groups still step, how many failed
__global__ void __launch_bounds__(256) rk45_status_kernel(const Rk45State* st, int G, Rk45Status* out) {
    __shared__ double red[256];
    double live = 0.0, failed = 0.0;
    for (int g = threadIdx.x; g < G; g += 256) {
        live += rk45_live(st[g]) ? 1.0 : 0.0;
        failed += st[g].failed ? 1.0 : 0.0;
    }
    const double rl = block_sum(live, red);
    __syncthreads();
    const double rf = block_sum(failed, red);
    if (threadIdx.x == 0) { out->unfinished = (int)rl; out->failed = (int)rf; }
}

__global__ void __launch_bounds__(256) rk45_out_kernel(const double* y, float* x, int n) {
    for (int i = 4 * (blockIdx.x * 256 + threadIdx.x); i < n; i += 4 * gridDim.x * 256) {
        double yv[4];
        load_y4(y, i, yv);
        *reinterpret_cast<float4*>(x + i) = make_float4((float)yv[0], (float)yv[1], (float)yv[2], (float)yv[3]);
    }
}

int rk45_chunks(int m, int cap) { int c = (m / 4 + 255) / 256; return c < 1 ? 1 : (c > cap ? cap : c); }

#define RK45_LAUNCH(kern, grid, ...)                                                                                   \
    do {                                                                                                               \
        if ((g.m & 3) || g.m < 4 || g.G < 1 || g.spg < 1 || g.chunks < 1)                                              \
            return fail(FC_E_SHAPE, "rk45: element count of a controller group must be a positive multiple of 4");     \
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, __VA_ARGS__);                                                  \
        FC_HIP(hipGetLastError());                                                                                     \
        return FC_OK;                                                                                                  \
    } while (0)
#define RK45_GRID dim3(g.chunks, g.G)

int rk45_setup_launch(const Rk45Groups& g, const float* x, double* y, float* xs, Rk45State* st, double t0, double t1, double rtol,
                      double atol, int max_attempts, float t_scale, float* tvec, int cfg_on, hipStream_t s) {
    RK45_LAUNCH(rk45_setup_kernel, RK45_GRID, x, y, xs, g.m, g.spg, st, t0, t1, rtol, atol, max_attempts, t_scale, tvec, cfg_on);
}
int rk45_d01_launch(const Rk45Groups& g, const Rk45State* st, const double* y, float* k0, const float* v2, int cfg_on, float cfg,
                    double* part, hipStream_t s) {
    RK45_LAUNCH(rk45_d01_kernel, RK45_GRID, st, y, k0, v2, g.m, cfg_on, cfg, part);
}
// `ll` (may be null): the likelihood's instantiation, which needs its whole record and takes no guidance pair
#define RK45_LL_CHECK                                                                                                   \
    if (ll && (!ll->a || !ll->d || ll->B != g.G * g.spg || ll->K < 1 || (ll->dk && !ll->ak) || (ll->K > 1 && !ll->dk))) return fail(FC_E_ARG, "rk45: the likelihood record does not fit the controller groups")
int rk45_h0_launch(const Rk45Groups& g, Rk45State* st, const double* part, float t_scale, float* tvec, int cfg_on, const Rk45LL* ll,
                   hipStream_t s) {
    RK45_LL_CHECK;
    if (ll) RK45_LAUNCH(rk45_h0_kernel<true>, dim3(g.G), st, part, g.chunks, g.m, g.spg, t_scale, tvec, cfg_on, *ll);
    RK45_LAUNCH(rk45_h0_kernel<false>, dim3(g.G), st, part, g.chunks, g.m, g.spg, t_scale, tvec, cfg_on, Rk45LL{});
}
int rk45_y1_launch(const Rk45Groups& g, const Rk45State* st, const double* y, const float* k0, float* xs, hipStream_t s) {
    RK45_LAUNCH(rk45_y1_kernel, RK45_GRID, st, y, k0, xs, g.m);
}
int rk45_d2_launch(const Rk45Groups& g, const Rk45State* st, const double* y, const float* k0, const float* v2, int cfg_on, float cfg,
                   double* part, hipStream_t s) {
    RK45_LAUNCH(rk45_d2_kernel, RK45_GRID, st, y, k0, v2, g.m, cfg_on, cfg, part);
}
int rk45_h1_launch(const Rk45Groups& g, Rk45State* st, const double* part, const Rk45LL* ll, hipStream_t s) {
    RK45_LL_CHECK;
    if (ll) RK45_LAUNCH(rk45_h1_kernel<true>, dim3(g.G), st, part, g.chunks, g.m, g.spg, *ll);
    RK45_LAUNCH(rk45_h1_kernel<false>, dim3(g.G), st, part, g.chunks, g.m, g.spg, Rk45LL{});
}
int rk45_stage_launch(const Rk45Groups& g, const Rk45State* st, int stage, const double* y, Rk45K kk, const float* v2, int cfg_on,
                      float cfg, float* xs, float t_scale, float* tvec, hipStream_t s) {
    switch (stage) {
        case 1: RK45_LAUNCH(rk45_stage_kernel<1>, RK45_GRID, st, y, kk, v2, g.m, g.spg, cfg_on, cfg, xs, t_scale, tvec);
        case 2: RK45_LAUNCH(rk45_stage_kernel<2>, RK45_GRID, st, y, kk, v2, g.m, g.spg, cfg_on, cfg, xs, t_scale, tvec);
        case 3: RK45_LAUNCH(rk45_stage_kernel<3>, RK45_GRID, st, y, kk, v2, g.m, g.spg, cfg_on, cfg, xs, t_scale, tvec);
        case 4: RK45_LAUNCH(rk45_stage_kernel<4>, RK45_GRID, st, y, kk, v2, g.m, g.spg, cfg_on, cfg, xs, t_scale, tvec);
        case 5: RK45_LAUNCH(rk45_stage_kernel<5>, RK45_GRID, st, y, kk, v2, g.m, g.spg, cfg_on, cfg, xs, t_scale, tvec);
        default: return fail(FC_E_ARG, "rk45: stage must lie in [1, 5]");
    }
}
int rk45_finish_launch(const Rk45Groups& g, const Rk45State* st, const double* y, double* y_new, Rk45K kk, const float* v2, int cfg_on,
                       float cfg, float* xs, float t_scale, float* tvec, hipStream_t s) {
    RK45_LAUNCH(rk45_finish_kernel, RK45_GRID, st, y, y_new, kk, v2, g.m, g.spg, cfg_on, cfg, xs, t_scale, tvec);
}
int rk45_error_launch(const Rk45Groups& g, const Rk45State* st, const double* y, const double* y_new, Rk45K kk, const float* v2,
                      int cfg_on, float cfg, double* part, hipStream_t s) {
    RK45_LAUNCH(rk45_error_kernel, RK45_GRID, st, y, y_new, kk, v2, g.m, cfg_on, cfg, part);
}
int rk45_control_launch(const Rk45Groups& g, Rk45State* st, const double* part, const Rk45Eval* ev, const Rk45LL* ll, hipStream_t s) {
    RK45_LL_CHECK;
    if (ll) RK45_LAUNCH(rk45_control_kernel<true>, dim3(g.G), st, part, g.chunks, g.m, g.spg, ev, *ll);
    RK45_LAUNCH(rk45_control_kernel<false>, dim3(g.G), st, part, g.chunks, g.m, g.spg, ev, Rk45LL{});
}
int rk45_dense_launch(const Rk45Groups& g, const Rk45State* st, const Rk45Eval* ev, const double* y, Rk45K kk, hipStream_t s) {
    if (!ev) return fail(FC_E_ARG, "rk45: dense output without a request record");
    RK45_LAUNCH(rk45_dense_kernel, RK45_GRID, st, ev, y, kk, g.m);
}
int rk45_commit_launch(const Rk45Groups& g, const Rk45State* st, double* y, const double* y_new, float* k0, const float* k6,
                       hipStream_t s) {
    RK45_LAUNCH(rk45_commit_kernel, RK45_GRID, st, y, y_new, k0, k6, g.m);
}
int rk45_status_launch(const Rk45Groups& g, const Rk45State* st, Rk45Status* out, hipStream_t s) {
    RK45_LAUNCH(rk45_status_kernel, dim3(1), st, g.G, out);
}
#undef RK45_LL_CHECK
#undef RK45_GRID
#undef RK45_LAUNCH

int rk45_out_launch(const double* y, float* x, int n, hipStream_t s) {
    if (n & 3) return fail(FC_E_SHAPE, "ode: element count must be a multiple of 4");
    hipLaunchKernelGGL(rk45_out_kernel, dim3(egrid(n)), dim3(256), 0, s, y, x, n);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

// ================================================================================================ likelihood on the RK4 grid
// fc_unet_log_likelihood: the RK4 step above (any grid direction; cfg off) carrying, per sample b, the integral of the Hutchinson
// divergence estimate next to x.  Every stage j has, besides its velocity v_j, the input gradient g_j = (dv_j/dx_j)^T eps of the same
// forward (fc_unet_vjp_x's chain); the kernel that closes the stage forms d_j[b] = sum_i eps[b,i] g_j[b,i] in the pass that does the
// state arithmetic, and the kernel that closes the interval adds (double(dt)/6)(d1 + 2 d2 + 2 d3 + d4) to a[b].
//
// One workgroup per sample: each thread's fp64 products are summed in index order, the 256 thread sums by block_sum's fixed tree, so
// d_j[b] depends on neither the batch size nor the scheduling, and no partial sums cross a launch.  (A sample is C*H*W <= a few 10^4
// floats, three streams of it per stage: the launches are latency-sized either way.)  That partition is why these are kernels of their
// own; the state arithmetic is ode_rk4_stage_kernel's / ode_rk4_final_kernel's by construction (rk4_stage_state, rk4_comb4, next_stage_tv).

// sum_i eps[base + i] g[base + i] over one sample, fp64 products and sums; the same value in every thread
__device__ __forceinline__ double probe_dot_acc(double s, const float4 e, const float4 q) {
    s += (double)e.x * (double)q.x; s += (double)e.y * (double)q.y;
    s += (double)e.z * (double)q.z; s += (double)e.w * (double)q.w;
    return s;
}

// K probes (layout: eps and g [K][B][m], dst [K][B][3], a [K][B], all strided by the call's B): the state arithmetic and probe 0's
// reduction share the first pass as they always did, probes 1..K-1 are reduced behind it by the same workgroup with the same loop and
// the same tree, so d_{j,k}[b] has the bits of a single-probe call with probe k.
__device__ __forceinline__ double probe_dot_sample(const float* eps, const float* g, int base, int m, double* red) {
    double d = 0.0;
    for (int j = 4 * threadIdx.x; j < m; j += 4 * 256)
        d = probe_dot_acc(d, *reinterpret_cast<const float4*>(eps + base + j), *reinterpret_cast<const float4*>(g + base + j));
    __syncthreads();   // the reduction before this one has been read
    return block_sum(d, red);
}

__global__ void __launch_bounds__(256) ode_ll_stage_kernel(const float* sc, const float* y, float* xs, float* k_out, const float* v,
                                                           const float* g, const float* eps, double* dst, int slot, int m, int full,
                                                           int tsel, float t_scale, float* tvec, int K) {
    __shared__ double red[256];
    const int b = blockIdx.x, base = b * m, B = gridDim.x;
    const float t = sc[0], dt = sc[1];
    if (threadIdx.x == 0) tvec[b] = next_stage_tv(t, dt, tsel, t_scale);
    double d = 0.0;
    for (int j = 4 * threadIdx.x; j < m; j += 4 * 256) {
        const int i = base + j;
        const float4 k = *reinterpret_cast<const float4*>(v + i);
        *reinterpret_cast<float4*>(k_out + i) = k;
        *reinterpret_cast<float4*>(xs + i) = rk4_stage_state(*reinterpret_cast<const float4*>(y + i), k, dt, full);
        d = probe_dot_acc(d, *reinterpret_cast<const float4*>(eps + i), *reinterpret_cast<const float4*>(g + i));
    }
    const double r = block_sum(d, red);
    if (threadIdx.x == 0) dst[3 * b + slot] = r;
    for (int k = 1; k < K; ++k) {
        const size_t pk = (size_t)k * B;
        const double rk = probe_dot_sample(eps + pk * m, g + pk * m, base, m, red);
        if (threadIdx.x == 0) dst[3 * (pk + b) + slot] = rk;
    }
}

// a + (dt/6)(d1 + 2 d2 + 2 d3 + d4), left to right
__device__ __forceinline__ double ll_interval_sum(double a, float dt, const double* ds, double d4) {
    return a + ((double)dt / 6.0) * (((ds[0] + 2.0 * ds[1]) + 2.0 * ds[2]) + d4);
}

__global__ void __launch_bounds__(256) ode_ll_final_kernel(const float* sc, float* y, const float* k1, const float* k2, const float* k3,
                                                           const float* v, const float* g, const float* eps, const double* dst, double* a,
                                                           int m, int K) {
    __shared__ double red[256];
    const int b = blockIdx.x, base = b * m, B = gridDim.x;
    const float dt6 = __fdiv_rn(sc[1], 6.0f);
    double d = 0.0;
    for (int j = 4 * threadIdx.x; j < m; j += 4 * 256) {
        const int i = base + j;
        const float4 k4 = *reinterpret_cast<const float4*>(v + i);
        const float4 p = *reinterpret_cast<const float4*>(k1 + i), q = *reinterpret_cast<const float4*>(k2 + i),
                     c = *reinterpret_cast<const float4*>(k3 + i);
        *reinterpret_cast<float4*>(y + i) = rk4_comb4(*reinterpret_cast<float4*>(y + i), p, q, c, k4, dt6);
        d = probe_dot_acc(d, *reinterpret_cast<const float4*>(eps + i), *reinterpret_cast<const float4*>(g + i));
    }
    const double d4 = block_sum(d, red);
    if (threadIdx.x == 0) a[b] = ll_interval_sum(a[b], sc[1], dst + 3 * b, d4);
    for (int k = 1; k < K; ++k) {
        const size_t pk = (size_t)k * B;
        const double dk = probe_dot_sample(eps + pk * m, g + pk * m, base, m, red);
        if (threadIdx.x == 0) a[pk + b] = ll_interval_sum(a[pk + b], sc[1], dst + 3 * (pk + b), dk);
    }
}

// The probes' mean and its standard error (thread b of an elementwise grid): abar[b] = (a_1[b] + ... + a_K[b]) / K, summed in probe
// order with one division; se[b] = sqrt(sum_k (a_k[b] - abar[b])^2 / (K (K - 1))), NaN for K = 1 (0 / 0).
// mean_given: abar[b] is the adaptive solve's own a and is read, not formed.
__global__ void __launch_bounds__(256) ode_ll_mean_kernel(const double* ak, int K, int B, double* abar, double* se, int mean_given) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    double mean;
    if (mean_given) mean = abar[b];
    else {
        double s = ak[b];
        for (int k = 1; k < K; ++k) s += ak[(size_t)k * B + b];
        abar[b] = mean = s / (double)K;
    }
    double q = 0.0;
    for (int k = 0; k < K; ++k) { const double e = ak[(size_t)k * B + b] - mean; q += e * e; }
    se[b] = sqrt(q / ((double)K * (double)(K - 1)));
}

// logp[b] = -|z_b|^2 / 2 - (m/2) ln(2 pi) + a[b]: the standard normal at the noise end plus the integrated divergence
__global__ void __launch_bounds__(256) ode_ll_logp_kernel(const float* z, const double* a, double* logp, int m) {
    __shared__ double red[256];
    const int b = blockIdx.x, base = b * m;
    double s = 0.0;
    for (int j = 4 * threadIdx.x; j < m; j += 4 * 256) s = probe_dot_acc(s, *reinterpret_cast<const float4*>(z + base + j), *reinterpret_cast<const float4*>(z + base + j));
    const double r = block_sum(s, red);
    if (threadIdx.x == 0) logp[b] = (-0.5 * r - 0.5 * (double)m * 1.8378770664093454835606594728112) + a[b];
}

// the stage kernels' reduction on its own (fc_debug_probe_dot's test hook with K = 1, dk = NULL), and behind every evaluation of the
// adaptive likelihood: for k in probe order dk[k][b] = sum eps_k g_k (eps, g [K][B][m]; dk [K][B], may be NULL for K = 1), then
// out[b] = (d_1 + ... + d_K) / K, summed in that order with one division (K = 1: the reduction itself)
__global__ void __launch_bounds__(256) ode_ll_dot_kernel(const float* eps, const float* g, double* out, double* dk, int m, int K) {
    __shared__ double red[256];
    const int b = blockIdx.x, base = b * m, B = gridDim.x;
    double d = 0.0;
    for (int j = 4 * threadIdx.x; j < m; j += 4 * 256)
        d = probe_dot_acc(d, *reinterpret_cast<const float4*>(eps + base + j), *reinterpret_cast<const float4*>(g + base + j));
    double r = block_sum(d, red);
    if (K == 1) {
        if (threadIdx.x == 0) { out[b] = r; if (dk) dk[b] = r; }
        return;
    }
    if (threadIdx.x == 0) dk[b] = r;
    for (int k = 1; k < K; ++k) {
        const size_t pk = (size_t)k * B;
        const double rk = probe_dot_sample(eps + pk * m, g + pk * m, base, m, red);
        if (threadIdx.x == 0) dk[pk + b] = rk;
        r += rk;
    }
    if (threadIdx.x == 0) out[b] = r / (double)K;
}

// probe k's slice starts at k * B * m: the whole [K][B][m] block is indexed with size_t, each slice with int
static int ll_probes_ok(int K, int B, int m) {
    (void)B; (void)m;
    if (K < 1 || K > FC_LL_MAX_PROBES) return fail(FC_E_ARG, "ode: the number of probes must lie in [1, " + std::to_string(FC_LL_MAX_PROBES) + "]");
    return FC_OK;
}
static int ll_shape_ok(int B, int m) {
    if (B < 1 || m < 4 || (m & 3)) return fail(FC_E_SHAPE, "ode: elements per sample must be a positive multiple of 4");
    if ((long long)B * m > 0x7fffffffLL) return fail(FC_E_SHAPE, "ode: the kernels index the batch with int (batch * elements per sample < 2^31)");
    return FC_OK;
}
int ode_ll_stage_launch(const float* sc, const float* y, float* xs, float* k_out, const float* v, const float* g, const float* eps,
                        double* dst, int slot, int B, int m, int full, int tsel, float t_scale, float* tvec, int K, hipStream_t s) {
    FC_TRY(ll_shape_ok(B, m));
    FC_TRY(ll_probes_ok(K, B, m));
    if (slot < 0 || slot > 2) return fail(FC_E_ARG, "ode: stage slot must lie in [0, 2]");
    if (tsel < 1 || tsel > 2) return fail(FC_E_ARG, "ode: the next stage's time selector must lie in [1, 2]");
    hipLaunchKernelGGL(ode_ll_stage_kernel, dim3(B), dim3(256), 0, s, sc, y, xs, k_out, v, g, eps, dst, slot, m, full, tsel, t_scale, tvec, K);
    FC_HIP(hipGetLastError());
    return FC_OK;
}
int ode_ll_final_launch(const float* sc, float* y, const float* k1, const float* k2, const float* k3, const float* v, const float* g,
                        const float* eps, const double* dst, double* a, int B, int m, int K, hipStream_t s) {
    FC_TRY(ll_shape_ok(B, m));
    FC_TRY(ll_probes_ok(K, B, m));
    hipLaunchKernelGGL(ode_ll_final_kernel, dim3(B), dim3(256), 0, s, sc, y, k1, k2, k3, v, g, eps, dst, a, m, K);
    FC_HIP(hipGetLastError());
    return FC_OK;
}
int ode_ll_logp_launch(const float* z, const double* a, double* logp, int B, int m, hipStream_t s) {
    FC_TRY(ll_shape_ok(B, m));
    hipLaunchKernelGGL(ode_ll_logp_kernel, dim3(B), dim3(256), 0, s, z, a, logp, m);
    FC_HIP(hipGetLastError());
    return FC_OK;
}
int ode_ll_dot_launch(const float* eps, const float* g, double* out, double* dk, int B, int m, int K, hipStream_t s) {
    FC_TRY(ll_shape_ok(B, m));
    FC_TRY(ll_probes_ok(K, B, m));
    if (K > 1 && !dk) return fail(FC_E_ARG, "ode: several probes need their per-probe rows");
    hipLaunchKernelGGL(ode_ll_dot_kernel, dim3(B), dim3(256), 0, s, eps, g, out, dk, m, K);
    FC_HIP(hipGetLastError());
    return FC_OK;
}
int ode_ll_mean_launch(const double* ak, int K, int B, double* abar, double* se, int mean_given, hipStream_t s) {
    if (K < 1 || K > FC_LL_MAX_PROBES || B < 1 || !ak || !abar || !se) return fail(FC_E_ARG, "ode: bad probe mean arguments");
    hipLaunchKernelGGL(ode_ll_mean_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, ak, K, B, abar, se, mean_given);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

// ================================================================================================ stochastic sampling (SDE)
// fc_unet_integrate_sde: the SDE with the marginals of the probability-flow ODE on the linear path x_t = (1-t) x0 + t x1 (DESIGN.md
// section 4b),
//     dx = b(x,t) dt + sigma sqrt(1-t) dW        b(x,t) = (1 + sigma^2 t / 2) v(x,t) - (sigma^2 / 2) x
// on the caller's grid.  Interval i, h = t1 - t0, a = sigma sqrt(h (1 - (t0 + t1)/2)) (the exact standard deviation of the noise integral),
// xi ~ N(0, I):
//     Euler-Maruyama   x+ = x + h b(x,t0) + a xi
//     Heun             xp = x + h b(x,t0) + a xi ;  x+ = x + (h/2)(b(x,t0) + b(xp,t1)) + a xi      (the same xi)
// Scalars: h, a, c1 = 1 + sigma^2 t / 2 (t = the evaluation's time) and c2 = sigma^2 / 2 are formed in fp64 from the fp32 grid entries and
// the fp32 sigma and rounded once to fp32; h/2 is exact.  Elementwise, single-rounded fp32 in this order: b = c1 v - c2 x (two products,
// one difference); x+ = (x + h b) + a xi; Heun's corrector (x + (h/2)(b1 + b2)) + a xi.  With sigma = 0: c1 = 1, c2 = 0, a = 0 and the
// step is deterministic Euler / Heun whatever xi.
//
// The noise field (flocoder_amd/noise.py is its host form): Philox4x32-10 with key (seed lo, seed hi) and counter (j, draw, sample id lo,
// sample id hi), j = the float4 group inside the sample's m elements, draw = the interval index counted from the call's first interval.
// The four output words r_k give u_k = ((r_k >> 9) + 0.5) 2^-23 (exact in fp32, in (0, 1)) and elements 4j .. 4j+3 are
//     R0 cos(pi w1), R0 sin(pi w1), R1 cos(pi w3), R1 sin(pi w3)       R = sqrt(-2 ln u) (logf, then a correctly rounded square root),
//     w = 2 u (exact), sincospif
// so |z| <= sqrt(48 ln 2) = 5.77 (u >= 2^-24).  A value depends on (seed, draw, sample id, position in the sample) alone: not on the row
// the sample sits in, the batch size or the launch geometry.

__device__ __forceinline__ float philox_u01(unsigned r) { return mul_(add_((float)(r >> 9), 0.5f), 1.1920928955078125e-07f); }   // 2^-23
__device__ __forceinline__ void box_muller(float u, float w_half, float* zc, float* zs) {
    const float R = __fsqrt_rn(mul_(-2.0f, logf(u)));
    float sn, cs;
    sincospif(mul_(2.0f, w_half), &sn, &cs);
    *zc = mul_(R, cs); *zs = mul_(R, sn);
}
__device__ __forceinline__ float4 normal4(unsigned long long seed, unsigned draw, unsigned long long sid, unsigned j) {
    unsigned r[4];
    philox4x32_10(j, draw, (unsigned)sid, (unsigned)(sid >> 32), (unsigned)seed, (unsigned)(seed >> 32), r);
    float4 z;
    box_muller(philox_u01(r[0]), philox_u01(r[1]), &z.x, &z.y);
    box_muller(philox_u01(r[2]), philox_u01(r[3]), &z.z, &z.w);
    return z;
}

// fc_ode_normal_field: out[b][4j .. 4j+3] of the field; sids == nullptr: sample id = b
__global__ void __launch_bounds__(256) ode_normal_field_kernel(float* out, unsigned long long seed, unsigned draw, const long long* sids,
                                                               int n, int m) {
    for (int i = 4 * (blockIdx.x * 256 + threadIdx.x); i < n; i += 4 * gridDim.x * 256) {
        const int b = i / m;
        const unsigned long long sid = sids ? (unsigned long long)sids[b] : (unsigned long long)b;
        *reinterpret_cast<float4*>(out + i) = normal4(seed, draw, sid, (unsigned)((i - b * m) >> 2));
    }
}

// fc_ode_probe_field, Rademacher: out[b][4j .. 4j+3] = +-1 from the top bit of the four words of the Philox block with counter
// (j, probe, sample id lo, sample id hi) -- a clear bit gives +1, a set one -1; `seed` is the caller's already offset key
__global__ void __launch_bounds__(256) ode_rademacher_field_kernel(float* out, unsigned long long seed, unsigned probe,
                                                                   const long long* sids, int n, int m) {
    for (int i = 4 * (blockIdx.x * 256 + threadIdx.x); i < n; i += 4 * gridDim.x * 256) {
        const int b = i / m;
        const unsigned long long sid = sids ? (unsigned long long)sids[b] : (unsigned long long)b;
        unsigned r[4];
        philox4x32_10((unsigned)((i - b * m) >> 2), probe, (unsigned)sid, (unsigned)(sid >> 32), (unsigned)seed, (unsigned)(seed >> 32), r);
        *reinterpret_cast<float4*>(out + i) = make_float4(r[0] >> 31 ? -1.0f : 1.0f, r[1] >> 31 ? -1.0f : 1.0f, r[2] >> 31 ? -1.0f : 1.0f,
                                                          r[3] >> 31 ? -1.0f : 1.0f);
    }
}

// fc_ode_probe_field, Gaussian: the normal field's uniforms and Box-Muller transform (same counter layout, same tail cut at
// sqrt(48 ln 2)) evaluated in fp64 and rounded once to fp32 -- what noise.probe_field computes on the host, so the two agree in bits
// wherever the fp64 log / sqrt / sin / cos of the two sides agree to well inside an fp32 rounding.  A probe field is drawn once per
// call, not once per interval like the sampler's noise: the fp64 transform costs nothing that shows.
__device__ __forceinline__ double philox_u01_f64(unsigned r) { return ((double)(r >> 9) + 0.5) * 1.1920928955078125e-07; }   // exact
__global__ void __launch_bounds__(256) ode_probe_normal_field_kernel(float* out, unsigned long long seed, unsigned probe,
                                                                     const long long* sids, int n, int m) {
    for (int i = 4 * (blockIdx.x * 256 + threadIdx.x); i < n; i += 4 * gridDim.x * 256) {
        const int b = i / m;
        const unsigned long long sid = sids ? (unsigned long long)sids[b] : (unsigned long long)b;
        unsigned r[4];
        philox4x32_10((unsigned)((i - b * m) >> 2), probe, (unsigned)sid, (unsigned)(sid >> 32), (unsigned)seed, (unsigned)(seed >> 32), r);
        const double two_pi = 2.0 * 3.141592653589793;
        const double r0 = sqrt(-2.0 * log(philox_u01_f64(r[0]))), r1 = sqrt(-2.0 * log(philox_u01_f64(r[2])));
        const double a0 = two_pi * philox_u01_f64(r[1]), a1 = two_pi * philox_u01_f64(r[3]);
        *reinterpret_cast<float4*>(out + i) = make_float4((float)(r0 * cos(a0)), (float)(r0 * sin(a0)), (float)(r1 * cos(a1)), (float)(r1 * sin(a1)));
    }
}

__device__ __forceinline__ float sde_drift(float c1, float c2, float v, float x) { return sub_(mul_(c1, v), mul_(c2, x)); }
__device__ __forceinline__ float sde_step(float x, float hb, float b, float a, float xi) { return add_(add_(x, mul_(hb, b)), mul_(a, xi)); }

// One launch behind each forward of an interval.  The interval index is *step - 1: ode_time_kernel opened the interval and moved the
// counter, so a captured interval is position-independent.  stage 0: Euler-Maruyama, y updated in place.  stage 1: Heun's predictor --
// b1 = b(y, t0) kept, xs = the predicted state, and block 0 publishes t1's scaled time rows for the second forward.  stage 2: Heun's
// corrector from v2 = v(xs, t1), y updated in place.  use_noise: xi is slice *step - 1 of prm->noise ([intervals][B][m] fp32) instead of
// the generated field.
__global__ void __launch_bounds__(256) ode_sde_update_kernel(const int* step, const float* ts, const SdeParams* prm, const long long* sids,
                                                             float* y, float* xs, float* b1, const float* v2, int n, int m, int cfg_on,
                                                             float cfg, float sigma, int stage, int use_noise, float t_scale, float* tvec,
                                                             int rows) {
    const int it = *step - 1;
    const float t0 = ts[it], t1 = ts[it + 1];
    if (stage == 1 && blockIdx.x == 0) {
        const float tv = mul_(t1, t_scale);
        for (int r = threadIdx.x; r < rows; r += 256) tvec[r] = tv;
    }
    const double hd = (double)t1 - (double)t0, s2 = 0.5 * (double)sigma * (double)sigma;
    const double rem = 1.0 - 0.5 * ((double)t0 + (double)t1);
    const float h = (float)hd, a = (float)((double)sigma * sqrt(hd * (rem > 0.0 ? rem : 0.0)));
    const float c1 = (float)(1.0 + s2 * (double)(stage == 2 ? t1 : t0)), c2 = (float)s2;
    const float hb = stage == 2 ? h * 0.5f : h;
    const unsigned long long seed = prm->seed;
    const float* xi_all = use_noise ? prm->noise + (size_t)it * (size_t)n : nullptr;
    for (int i = 4 * (blockIdx.x * 256 + threadIdx.x); i < n; i += 4 * gridDim.x * 256) {
        const float4 v = load_v(v2, i, n, cfg_on, cfg);
        const float4 yv = *reinterpret_cast<const float4*>(y + i);
        float4 xi;
        if (xi_all) xi = *reinterpret_cast<const float4*>(xi_all + i);
        else {
            const int b = i / m;
            xi = normal4(seed, (unsigned)it, (unsigned long long)sids[b], (unsigned)((i - b * m) >> 2));
        }
        float4 bv, o;
        if (stage == 2) {
            const float4 xp = *reinterpret_cast<const float4*>(xs + i), p = *reinterpret_cast<const float4*>(b1 + i);
            bv.x = add_(p.x, sde_drift(c1, c2, v.x, xp.x)); bv.y = add_(p.y, sde_drift(c1, c2, v.y, xp.y));      // b1 + b2
            bv.z = add_(p.z, sde_drift(c1, c2, v.z, xp.z)); bv.w = add_(p.w, sde_drift(c1, c2, v.w, xp.w));
        } else {
            bv.x = sde_drift(c1, c2, v.x, yv.x); bv.y = sde_drift(c1, c2, v.y, yv.y);
            bv.z = sde_drift(c1, c2, v.z, yv.z); bv.w = sde_drift(c1, c2, v.w, yv.w);
            if (stage == 1) *reinterpret_cast<float4*>(b1 + i) = bv;
        }
        o.x = sde_step(yv.x, hb, bv.x, a, xi.x); o.y = sde_step(yv.y, hb, bv.y, a, xi.y);
        o.z = sde_step(yv.z, hb, bv.z, a, xi.z); o.w = sde_step(yv.w, hb, bv.w, a, xi.w);
        *reinterpret_cast<float4*>((stage == 1 ? xs : y) + i) = o;
    }
}

// sample ids of a call that passes none: 0 .. B-1
__global__ void __launch_bounds__(256) ode_iota_kernel(long long* ids, int B) {
    for (int b = blockIdx.x * 256 + threadIdx.x; b < B; b += gridDim.x * 256) ids[b] = b;
}

static int sde_shape_ok(int n, int m) {
    if (n < 4 || m < 4 || (m & 3) || n % m) return fail(FC_E_SHAPE, "ode: elements per sample must be a positive multiple of 4 and divide the batch's");
    return FC_OK;
}
int ode_normal_field_launch(float* out, unsigned long long seed, unsigned draw, const int64_t* sids, int n, int m, hipStream_t s) {
    FC_TRY(sde_shape_ok(n, m));
    hipLaunchKernelGGL(ode_normal_field_kernel, dim3(egrid(n)), dim3(256), 0, s, out, seed, draw, reinterpret_cast<const long long*>(sids), n, m);
    FC_HIP(hipGetLastError());
    return FC_OK;
}
int ode_sde_update_launch(const int* step, const float* ts, const SdeParams* prm, const int64_t* sids, float* y, float* xs, float* b1,
                          const float* v2, int n, int m, int cfg_on, float cfg, float sigma, int stage, int use_noise, float t_scale,
                          float* tvec, int rows, hipStream_t s) {
    FC_TRY(sde_shape_ok(n, m));
    if (stage < 0 || stage > 2) return fail(FC_E_ARG, "ode: SDE stage must lie in [0, 2]");
    hipLaunchKernelGGL(ode_sde_update_kernel, dim3(egrid(n)), dim3(256), 0, s, step, ts, prm,
                       reinterpret_cast<const long long*>(sids), y, xs, b1, v2, n, m, cfg_on, cfg, sigma, stage, use_noise, t_scale, tvec, rows);
    FC_HIP(hipGetLastError());
    return FC_OK;
}
int ode_probe_normal_field_launch(float* out, unsigned long long seed, unsigned probe, const int64_t* sids, int n, int m, hipStream_t s) {
    FC_TRY(sde_shape_ok(n, m));
    hipLaunchKernelGGL(ode_probe_normal_field_kernel, dim3(egrid(n)), dim3(256), 0, s, out, seed, probe, reinterpret_cast<const long long*>(sids), n, m);
    FC_HIP(hipGetLastError());
    return FC_OK;
}
int ode_rademacher_field_launch(float* out, unsigned long long seed, unsigned probe, const int64_t* sids, int n, int m, hipStream_t s) {
    FC_TRY(sde_shape_ok(n, m));
    hipLaunchKernelGGL(ode_rademacher_field_kernel, dim3(egrid(n)), dim3(256), 0, s, out, seed, probe, reinterpret_cast<const long long*>(sids), n, m);
    FC_HIP(hipGetLastError());
    return FC_OK;
}
int ode_iota_launch(int64_t* ids, int B, hipStream_t s) {
    hipLaunchKernelGGL(ode_iota_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, reinterpret_cast<long long*>(ids), B);
    FC_HIP(hipGetLastError());
    return FC_OK;
}

}  // namespace fc
