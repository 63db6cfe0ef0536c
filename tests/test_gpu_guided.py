"""Measurement-guided RK4 sampling on the GPU (fc_ode_guided_correct, fc_unet_integrate_guided) against the fp64 formula and the fp64
restatement over the oracle U-Net (tests/guided_ref.py).  Cases: tests/guided_ref.py CASES (the likelihood test's models).

Gates, none of them measured on the code under test:
  one correction   per element, from the documented operation sequence (ode.hip guide_w / guide_apply): eleven
                   single-rounded fp32 operations and four scalars rounded once from fp64.  With u = 2^-24, c = gamma (1-t)/t,
                   X = |x| + |(1-t) v|, M = |a| (|y| + |a| X), den = r2 a^2 + sigma_y^2, first-order propagation gives
                       x1: 3u X;  a x1, res, a res: 6u M in all;  den: 4u den;  w = num / den: (6 + 4 + 1) u M / den;
                       c w: + 2u |c| M / den;  v + c w: + u (|v| + |c| M / den)         => 14u |c| M / den + u |v|,
                   and the gate is N u (|v| + |c| M / den) with N = 15, the number of rounded quantities (second-order terms covered).
                   Where the denominator is exactly 0 (a = 0 and sigma_y = 0) and where the correction term is 0, out must EQUAL v.
  no correction    gamma = 0, and keep = 0: torch.equal to generate_latents_rk4(init_latents=..., init_strength=...)
  trajectories     per-sample relative L2 < TRAJ_TOL = 2e-4 against the restatement, both Jacobian modes (tests/test_gpu_unet.py's gate)
  chain term       torch.equal to Unet.vjp_x on the same stage state, time and cotangent
With -s every case prints its figures.

Measured on the MI355X (worst sample per case, cases in CASES order; also in DESIGN.md section 4):
  one correction           at most 0.32 of the bound
  identity / restatement   1.4e-6, 8.3e-7, 8.1e-7, 5.2e-7 relative; without graphs (child process, first case) 1.4e-6
  exact / restatement      2.7e-6, 1.6e-6, 8.4e-6, 5.4e-6
  kept-region residual     unguided 46-56, 40-41, 77, 27-28; identity 4.1-5.5, 3.1-3.3, 9.3-9.8, 2.2-2.4; exact vs identity 33-97 % apart"""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import guided_ref as gr
from conftest import ROOT
from oracle import flow_oracle as fo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRAJ_TOL = 2e-4
U = 2.0 ** -24
N_OPS = 15
_REF = {}


def _ref(cid):
    if cid not in _REF:
        _REF[cid] = gr.case_refs(cid)
    return _REF[cid]


def _model(sd, train=False):
    from flocoder_amd.unet import Unet
    m = fo.unet_meta(sd)
    model = Unet(dim=m["dim"], dim_mults=(1, 2, 4, 8), channels=4, n_classes=m["n_classes"], mask_cond=m["mask_cond"])
    model.load_state_dict(sd, strict=True)
    return model.to(DEV).train(train)


def _dev(cond):
    return None if cond is None else {k: v.to(DEV) for k, v in cond.items()}


def _rel(a, b):
    a, b = a.double().cpu().flatten(1), b.double().cpu().flatten(1)
    return (a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-300)


def _guided(model, c, jacobian="identity", cfg=None, **kw):
    from flocoder_amd import sampling as S
    shape = tuple(c["source"].shape)
    args = dict(n_steps=c["n"], init_strength=gr.INIT_STRENGTH, cond=_dev(c["cond"]), cfg_strength=c["cfg"] if cfg is None else cfg,
                source=c["source"].to(DEV), sigma_y=gr.SIGMA_Y, gamma=gr.GAMMA, jacobian=jacobian)
    args.update(kw)
    keep = args.pop("keep", c["keep"]).to(DEV)
    lat, nfe = S.generate_latents_guided(model, shape, c["measurement"].to(DEV), keep, **args)
    torch.cuda.synchronize()
    return lat, nfe


def _plain(model, c, cfg=None):
    from flocoder_amd import sampling as S
    lat, nfe = S.generate_latents_rk4(model, tuple(c["source"].shape), c["n"], _dev(c["cond"]), c["cfg"] if cfg is None else cfg,
                                      source=c["source"].to(DEV), init_latents=c["measurement"].to(DEV), init_strength=gr.INIT_STRENGTH)
    torch.cuda.synchronize()
    return lat, nfe


def test_one_correction_against_the_fp64_formula_within_the_derived_bound():
    from flocoder_amd import _binding as B
    from oracle.synth import synth_input
    n = 4 * 33 * 64
    v, x, known = (synth_input(f"guided.k.{s}", (n,), 11) for s in "vxk")
    u01 = torch.sigmoid(synth_input("guided.k.a", (n,), 11))
    a = torch.where(u01 < 0.3, torch.zeros_like(u01), torch.where(u01 > 0.6, torch.ones_like(u01), u01))       # 0, fractional and 1
    y = a * known
    vd, xd, yd, ad = (t.to(DEV).contiguous() for t in (v, x, y, a))
    worst = 0.0
    t_half = float(torch.tensor(0.2, dtype=torch.float32) + torch.tensor(0.35, dtype=torch.float32) * 0.5)
    for t in (0.296, t_half, 0.5, 0.97, 1.0):
        for sy in (0.05, 0.5, 0.0):
            for gam in (1.0, 0.5, 0.0):
                out = torch.empty_like(vd)
                B.check(B.lib().fc_ode_guided_correct(B.ptr(vd), B.ptr(xd), B.ptr(yd), B.ptr(ad), n, t, sy, gam, B.ptr(out),
                                                      B.current_stream(vd.device)))
                torch.cuda.synchronize()
                t64 = float(torch.tensor(t, dtype=torch.float32))                       # what the kernel was given
                s64, g64 = float(torch.tensor(sy, dtype=torch.float32)), float(torch.tensor(gam, dtype=torch.float32))
                V, X, Y, A = v.double(), x.double(), y.double(), a.double()
                ref = gr.correct(V, X, torch.tensor(t64, dtype=torch.float64), Y, A, s64, g64)
                om = 1 - t64
                c = abs(g64 * om / t64)
                den = om * om / (t64 * t64 + om * om) * A * A + s64 * s64
                M = A * (Y.abs() + A * (X.abs() + (om * V).abs()))
                zero = den == 0
                bound = N_OPS * U * (V.abs() + c * M / torch.where(zero, torch.ones_like(den), den))
                err = (out.cpu().double() - ref).abs()
                ratio = float((err[~zero] / bound[~zero].clamp_min(1e-300)).max()) if bool((~zero).any()) else 0.0
                worst = max(worst, ratio)
                assert bool((err[~zero] <= bound[~zero]).all()), (t, sy, gam, ratio)
                assert torch.equal(out.cpu()[zero], v[zero]), (t, sy, gam)
                if gam == 0.0 or t == 1.0:
                    assert torch.equal(out.cpu(), v), (t, sy, gam)
                else:
                    assert not torch.equal(out.cpu(), v)
    print(f"\nworst |out - fp64| / bound over all (t, sigma_y, gamma): {worst:.3f}")
    bad = torch.empty(n + 1, device=DEV)[1:]
    with pytest.raises(ValueError, match="aligned"):
        B.check(B.lib().fc_ode_guided_correct(B.ptr(bad), B.ptr(xd), B.ptr(yd), B.ptr(ad), n, 0.5, 0.05, 1.0, B.ptr(vd.clone()), B.current_stream(vd.device)))
    for t, sy in ((0.0, 0.05), (-1.0, 0.05), (0.5, -0.1)):
        with pytest.raises(ValueError):
            B.check(B.lib().fc_ode_guided_correct(B.ptr(vd), B.ptr(xd), B.ptr(yd), B.ptr(ad), n, t, sy, 1.0, B.ptr(vd.clone()), B.current_stream(vd.device)))


@pytest.mark.parametrize("cid", list(gr.CASES))
def test_without_correction_the_bits_are_the_plain_samplers(cid):
    """gamma = 0, and keep = 0 (the full-shape and the [B,1,H,W] form): torch.equal to generate_latents_rk4 from the same start; and a plain
    sampler call AFTER guided calls on the same model gives the bits of a model that never ran one (graphs and buffers are apart)."""
    c = gr.case_inputs(cid)
    used, fresh = _model(c["sd"]), _model(c["sd"])
    plain, nfe0 = _plain(fresh, c)
    g0, nfe = _guided(used, c, gamma=0.0)
    assert nfe == nfe0 and torch.equal(g0, plain)
    k0, _ = _guided(used, c, keep=torch.zeros_like(c["keep"]))
    assert torch.equal(k0, plain)
    k1, _ = _guided(used, c, keep=torch.zeros_like(c["source"]), sigma_y=0.0)
    assert torch.equal(k1, plain)
    live, _ = _guided(used, c)
    assert torch.isfinite(live).all() and float(_rel(live, plain).min()) > 1e-2
    again, _ = _plain(used, c)
    assert torch.equal(again, plain)
    assert used.launches_per_forward == fresh.launches_per_forward


_CHILD = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import torch
import guided_ref as gr
import test_gpu_guided as T
c = gr.case_inputs("d16c10-class-cfg3")
m = T._model(c["sd"])
plain, _ = T._plain(T._model(c["sd"]), c)
g0, _ = T._guided(m, c, gamma=0.0)
k0, _ = T._guided(m, c, keep=torch.zeros_like(c["keep"]))
live, _ = T._guided(m, c)
ref = gr.case_refs("d16c10-class-cfg3", ("identity",))["identity"].latents
print("RESULT", int(torch.equal(g0, plain)), int(torch.equal(k0, plain)), float(T._rel(live, ref).max()))
"""


@pytest.mark.timeout(900)
def test_direct_launches_without_graphs_in_a_child_process():
    """FLOCODER_AMD_NO_GRAPH set (read once per process, hence the child): the same equalities and the trajectory gate for one case."""
    env = dict(os.environ)
    env["FLOCODER_AMD_NO_GRAPH"] = "1"
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=800, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")]
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    _, e0, e1, rel = lines[-1].split()
    print(f"\nno-graph child: gamma=0 equal {e0}, keep=0 equal {e1}, guided rel-L2 to the restatement {rel}")
    assert e0 == "1" and e1 == "1" and float(rel) < TRAJ_TOL


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("cid", list(gr.CASES))
def test_both_modes_match_the_fp64_restatement_and_pull_towards_the_measurement(cid):
    c = gr.case_inputs(cid)
    ref = _ref(cid)
    model = _model(c["sd"])
    ident, nfe = _guided(model, c)
    exact, nfe_e = _guided(model, c, jacobian="exact", cfg=0.0)
    ident0 = ident if not c["cfg"] else _guided(model, c, cfg=0.0)[0]
    plain, _ = _plain(model, c)
    assert nfe == nfe_e == 4 * max(1, int(c["n"] * (1 - gr.INIT_STRENGTH))) and not model.training
    assert all(p.grad is None for p in model.parameters())
    ri, re_ = _rel(ident, ref["identity"].latents), _rel(exact, ref["exact"].latents)
    rp = _rel(plain, ref["unguided"])
    res_g, res_e = gr.kept_residual(ident.cpu(), c["keep"], c["known"]), gr.kept_residual(exact.cpu(), c["keep"], c["known"])
    res_u = gr.kept_residual(plain.cpu(), c["keep"], c["known"])
    diff = _rel(exact, ident0)
    print(f"\n[{cid}] rel-L2 to the restatement: identity {ri.tolist()}, exact {re_.tolist()}, plain sampler {rp.tolist()}; kept-region residual "
          f"guided {res_g.tolist()}, exact {res_e.tolist()}, unguided {res_u.tolist()}; exact vs identity rel-L2 {diff.tolist()}")
    assert torch.isfinite(ident).all() and torch.isfinite(exact).all()
    assert float(ri.max()) < TRAJ_TOL, ri
    assert float(re_.max()) < TRAJ_TOL, re_
    assert bool((res_g < res_u).all()), (res_g, res_u)
    assert float(diff.min()) > TRAJ_TOL, diff


def _peek(ptr, shape, dtype=torch.float32):
    from flocoder_amd import _binding as B
    out = torch.empty(shape, dtype=dtype, device=DEV)
    B.check(B.lib().fc_debug_copy(B.ptr(out), ptr, out.numel() * out.element_size(), B.current_stream(out.device)))
    torch.cuda.synchronize()
    return out


def test_exact_mode_chain_term_is_vjp_x_and_refusals():
    """One interval in the exact form; the last stage's input state, scaled time, w and q are read back from the library's buffers, and the
    same state through a training forward and Unet.vjp_x with that w gives q's bits (the same plan entries on the same kind of buffers)."""
    from flocoder_amd import _binding as B
    c = gr.case_inputs("d16c10-nocond")
    c2 = gr.case_inputs("d16c10-class-cfg3")
    model = _model(c2["sd"])
    cls = c2["cond"]["class_cond"].to(DEV)
    x = c["source"].to(DEV).clone()
    ts = torch.tensor([0.3, 0.55], dtype=torch.float32)
    y, keep = c["measurement"].to(DEV), c["keep"].to(DEV)
    with pytest.raises(ValueError, match="guidance"):
        model.integrate_guided(x.clone(), ts, y, keep, jacobian="exact", class_ids=cls, cfg_strength=3.0)
    with pytest.raises(ValueError, match="> 0"):
        model.integrate_guided(x.clone(), torch.tensor([0.0, 0.5]), y, keep)
    with pytest.raises(ValueError, match="sigma_y"):
        model.integrate_guided(x.clone(), ts, y, keep, sigma_y=-0.1)
    # the native entry refuses the exact form on a handle without the backward plan
    model.reserve(3, 16, 16)
    kp = keep.expand_as(x).contiguous()
    tsh = ts.numpy().ctypes.data_as(C.POINTER(C.c_float))
    rc = B.lib().fc_unet_integrate_guided(model._handle, B.ptr(x.clone()), 3, 16, 16, tsh, 2, 999.0, B.ptr(cls), 0.0, None, 0, B.ptr(y), B.ptr(kp),
                                          0.05, 1.0, B.FC_JACOBIAN_EXACT, B.current_stream(x.device))
    assert rc == B.FC_E_STATE
    rc = B.lib().fc_unet_integrate_guided(model._handle, B.ptr(x.clone()), 3, 16, 16, tsh, 2, 999.0, B.ptr(cls), 0.0, None, 0, B.ptr(y),
                                          kp.data_ptr() + 4, 0.05, 1.0, B.FC_JACOBIAN_IDENTITY, B.current_stream(x.device))
    assert rc == B.FC_E_ARG

    model.integrate_guided(x, ts, y, keep, jacobian="exact", class_ids=cls, restore_plan=False)
    torch.cuda.synchronize()
    assert B.lib().fc_unet_train_form(model._handle) == 1
    px, pt, pw, pq = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    B.check(B.lib().fc_debug_unet_guided_buffers(model._handle, C.byref(px), C.byref(pt), C.byref(pw), C.byref(pq)))
    xs, tv, w, q = _peek(px.value, x.shape), _peek(pt.value, (3,)), _peek(pw.value, x.shape), _peek(pq.value, x.shape)
    t_last = (ts[0] + (ts[1] - ts[0])) * 999.0                                  # t + dt, then * t_scale: the stage kernels' operations
    assert torch.equal(tv.cpu(), t_last.expand(3))
    assert torch.isfinite(q).all() and float(w.abs().max()) > 0 and float(q.abs().max()) > 0
    v = model._forward_native(xs, tv, cls, None, train=True)
    q2 = model.vjp_x(xs, tv, cls, w)
    torch.cuda.synchronize()
    assert torch.equal(q2, q)
    # w itself is the documented sequence on (v, xs): the one-evaluation entry gives v + c w, compared through the fp64 formula's bound
    t64 = float(ts[0] + (ts[1] - ts[0]))
    w64 = gr.weight(v.double().cpu(), xs.double().cpu(), torch.tensor(t64, dtype=torch.float64), y.double().cpu(), keep.double().cpu(), 0.05)
    assert float((w.double().cpu() - w64).abs().max()) <= 16 * U * float(w64.abs().max() + 1) * 400      # 1 / sigma_y^2 = 400 scales the residual's rounding
    model.release_training_plan()
    assert B.lib().fc_unet_train_form(model._handle) == 0


@pytest.mark.timeout(900)
def test_an_exact_call_leaks_nothing_into_sampling_or_training():
    """After an exact-form call a model that was sampling has its inference plans and reservation back: a sampler call gives a fresh model's
    bits.  A guided call (either form) between two FlowTrainer steps leaves the second step bit-equal to a run without it."""
    from flocoder_amd import _binding as B
    from flocoder_amd.train import FlowTrainer
    from flocoder_amd.unet import Unet
    from conftest import load_golden
    from oracle.synth import synth_input, synth_state_dict
    c = gr.case_inputs("d16c10-class-cfg3")
    used, fresh = _model(c["sd"]), _model(c["sd"])
    used.reserve(12, 16, 16)
    n_inf = used.launches_per_forward
    e1, _ = _guided(used, c, jacobian="exact", cfg=0.0)
    assert B.lib().fc_unet_train_form(used._handle) == 0 and used.chains[1] == 12 and used.launches_per_forward == n_inf
    e2, _ = _guided(used, c, jacobian="exact", cfg=0.0)
    assert torch.equal(e1, e2)
    used.reserve(6, 16, 16)
    a, _ = _plain(used, c)
    b, _ = _plain(fresh, c)
    assert torch.equal(a, b) and used.launches_per_forward == fresh.launches_per_forward

    g = load_golden("g10_train_step")
    sd = synth_state_dict(g["shapes"], 10)
    cls = torch.from_numpy(g["cls"]).to(DEV)
    xg, known = synth_input("guided.hyg.x", (8, 4, 16, 16), 1).to(DEV), synth_input("guided.hyg.k", (8, 4, 16, 16), 1).to(DEV)
    keep = (synth_input("guided.hyg.a", (8, 1, 16, 16), 1) > 0).float().to(DEV)

    def run(jac):
        from flocoder_amd import sampling as S
        m = Unet(dim=16, channels=4, dim_mults=(1, 2, 4, 8), n_classes=10)
        m.load_state_dict(sd)
        tr = FlowTrainer(m.to(DEV).train(), lr=1e-4)
        out = []
        for step in (1, 2):
            src, tgt = synth_input(f"g10.src{step}", (8, 4, 16, 16), 10), synth_input(f"g10.tgt{step}", (8, 4, 16, 16), 10)
            u = torch.sigmoid(synth_input(f"g10.u{step}", (8,), 10, scale=1.5))
            loss = tr.step(src.to(DEV), tgt.to(DEV), {"class_cond": cls, "mask_cond": None}, u=u.to(DEV))
            out.append((loss.clone(), tr.grads.clone(), tr.params.clone()))
            if jac and step == 1:
                serial = m.arena_serial()
                lat, _ = S.generate_latents_guided(m, (8, 4, 16, 16), keep * known, keep, n_steps=4, cond={"class_cond": cls}, cfg_strength=0.0,
                                                   source=xg, jacobian=jac)
                assert m.arena_serial() != serial and m.training and torch.isfinite(lat).all()
        torch.cuda.synchronize()
        return out

    plain = run(None)
    for jac in ("exact", "identity"):
        for (l0, g0, p0), (l1, g1, p1) in zip(plain, run(jac)):
            assert torch.equal(l0, l1) and torch.equal(g0, g1) and torch.equal(p0, p1), jac
