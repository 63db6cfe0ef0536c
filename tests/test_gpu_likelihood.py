"""Flow log-likelihood and latent inversion on the GPU (fc_unet_vjp_x, fc_unet_log_likelihood) against the fp64 restatement over the
oracle U-Net (tests/likelihood_ref.py).

Gates, none of them measured on the code under test:
  z      per-sample relative L2 < TRAJ_TOL = 2e-4, the trajectory gate of tests/test_gpu_unet.py (these cases make 16 or 32 forwards)
  a      |a_gpu[b] - a_64[b]| <= G_TOL |eps_b| sum_intervals (|dt|/6)(|g1| + 2|g2| + 2|g3| + |g4|)_b from the reference's own g_j: the
         per-sample d(x) gate of tests/unet_grad_taps.py (G_TOL = 2e-6) through Cauchy-Schwarz
  logp   that bound plus |(|z_gpu|^2 - |z_64|^2)| / 2 from the two z
  d_j    one evaluation at the reference's own stage state: |d_gpu - d_64| <= G_TOL |eps_b| |g_j|_b
With -s every case prints its worst |a_gpu - a_64| / bound.

Measured on the MI355X (worst sample per case; also in DESIGN.md section 4):
  |a_gpu - a_64| / bound   d16c10-class 0.024, d16c10-nocond 0.010, d32c102-class 0.013, d8mask 0.015, d8mask-ones 0.005, d16c10-B5-of-8 0.020
  |logp_gpu - logp_64|     at most 0.21 of its bound (d32c102-class)
  z                        at most 5.1e-7 relative; invert_latents at most 4.9e-7 against the restatement, 1.8e-7 against log_likelihood's z
  one evaluation           d_j at most 0.106 of its bound over the four stages of interval 0; at stage 1 (t = 1) v is 4e-6 and g 5-7e-6 from
                           the fp64 ones (fp32 time sinusoid), 2e-6 / 2.5e-6 at the later stages
"""
import ctypes as C
import math
import re

import pytest
import torch

import likelihood_ref as lr
from conftest import load_golden
from oracle import flow_oracle as fo
from oracle.synth import synth_input, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G_TOL = 2e-6
TRAJ_TOL = 2e-4

PARAM_ONLY = {"conv_wgrad", "conv_wgrad_table", "wgrad_reduce", "norm_param_grads", "dense_bwd_w", "time_mlp_bwd", "class_mlp_bwd",
              "finalize", "finalize_table"}

# id: (shape table, seed, B, H = W, conditioning, n_steps, rows the plan is reserved for before the call (0: the call's own))
CASES = {
    "d16c10-class": ("d16c10", 2, 3, 16, "class", 9, 0),
    "d16c10-nocond": ("d16c10", 2, 3, 16, None, 9, 0),
    "d32c102-class": ("d32c102", 1, 2, 32, "class", 5, 0),
    "d8mask": ("d8mask", 3, 3, 8, "mask", 9, 0),
    "d8mask-ones": ("d8mask", 3, 3, 8, "mask-ones", 9, 0),
    "d16c10-B5-of-8": ("d16c10", 2, 5, 16, "class", 5, 8),
}
_REF = {}


def _inputs(cid):
    tag, seed, bsz, hw, kind, n, reserve = CASES[cid]
    sd = synth_state_dict(load_golden("g3_unet_" + tag)["shapes"], seed)
    meta = fo.unet_meta(sd)
    g = torch.Generator().manual_seed(3000 + seed)
    x = synth_input(f"ll.x.{cid}", (bsz, 4, hw, hw), seed)
    eps = torch.where(synth_input(f"ll.eps.{cid}", (bsz, 4, hw, hw), seed) >= 0, 1.0, -1.0)
    cond = {}
    if kind == "class":
        cond["class_cond"] = torch.randint(0, meta["n_classes"], (bsz,), generator=g)
    elif kind == "mask":
        cond["mask_cond"] = (torch.rand(bsz, 4, hw, hw, generator=g) > 0.35).float()
    elif kind == "mask-ones":
        cond["mask_cond"] = torch.ones(bsz, 4, hw, hw)
    return sd, x, eps, (cond or None), n, reserve


def _ref(cid):
    if cid not in _REF:
        sd, x, eps, cond, n, _ = _inputs(cid)
        sd64 = {k: v.double() for k, v in sd.items()}
        _REF[cid] = lr.log_likelihood_ref(sd64, x.double(), n, cond, eps.double())
    return _REF[cid]


def _model(sd, train=True):
    from flocoder_amd.unet import Unet
    m = fo.unet_meta(sd)
    model = Unet(dim=m["dim"], dim_mults=(1, 2, 4, 8), channels=4, n_classes=m["n_classes"], mask_cond=m["mask_cond"])
    model.load_state_dict(sd, strict=True)
    return model.to(DEV).train(train)


def _dev_cond(cond):
    return None if cond is None else {k: v.to(DEV) for k, v in cond.items()}


def _reserve_rows(model, rows, hw):
    model._forward_native(torch.zeros(rows, 4, hw, hw, device=DEV), torch.zeros(rows, device=DEV), None, None, train=True)


def _backward_forms(model):
    from flocoder_amd import _binding as B
    lib = B.lib()
    out = []
    for i in range(lib.fc_unet_backward_launches(model._handle)):
        k, m = C.c_char_p(), C.c_char_p()
        B.check(lib.fc_unet_backward_op_info(model._handle, i, C.byref(k), C.byref(m)))
        out.append((k.value.decode(), m.value.decode()))
    return out


def _rel(a, b):
    a, b = a.double().cpu().flatten(1), b.double().cpu().flatten(1)
    return (a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-300)


def _probe_dot(eps, g):
    from flocoder_amd import _binding as B
    out = torch.empty(eps.shape[0], dtype=torch.float64, device=eps.device)
    B.check(B.lib().fc_debug_probe_dot(B.ptr(eps), B.ptr(g), B.ptr(out), eps.shape[0], eps[0].numel(), B.current_stream(eps.device)))
    return out


@pytest.mark.parametrize("cid", list(CASES))
def test_vjp_x_is_the_backwards_dx_and_runs_no_parameter_only_launch(cid):
    """d(x) from the data-gradient chain alone has the bits of the full backward's d(x) (no summation order changes when launches that
    feed nothing on the chain are left out); it leaves a flat gradient vector alone; its launch list names no parameter-only kernel and
    is shorter than the backward's, which stays what it was."""
    from flocoder_amd import _binding as B
    sd, x, eps, cond, n, reserve = _inputs(cid)
    model = _model(sd)
    bsz, hw = x.shape[0], x.shape[-1]
    if reserve:
        _reserve_rows(model, reserve, hw)
    xd, ed = x.to(DEV), eps.to(DEV)
    td = (torch.rand(bsz, generator=torch.Generator().manual_seed(5)) * 999).to(DEV)
    cd = None if not cond or "class_cond" not in cond else cond["class_cond"].to(DEV)
    md = None if not cond or "mask_cond" not in cond else cond["mask_cond"].to(DEV)
    model._forward_native(xd, td, cd, md, train=True)
    forms0, count0 = _backward_forms(model), B.lib().fc_unet_backward_launches(model._handle)
    dx_a = model.vjp_x(xd, td, cd, ed, mask=md)
    flat, dx_b, _ = model.backward_native(xd, td, cd, ed, mask=md, want_dx=True)
    keep = flat.clone()
    dx_c = model.vjp_x(xd, td, cd, ed, mask=md)
    torch.cuda.synchronize()
    assert torch.isfinite(dx_a).all() and float(dx_a.abs().max()) > 0
    assert torch.equal(dx_a, dx_b) and torch.equal(dx_c, dx_b)
    assert torch.equal(flat, keep) and float(flat.abs().max()) > 0
    vj = model.vjp_forms()
    names = {re.sub(r"<[^>]*>", "", k) for k, _ in vj}
    assert not (names & PARAM_ONLY), sorted(names & PARAM_ONLY)
    assert 0 < len(vj) < count0 and len(vj) == B.lib().fc_unet_vjp_launches(model._handle)
    assert B.lib().fc_unet_backward_launches(model._handle) == count0 and _backward_forms(model) == forms0
    assert {"gn_bwd", "dgrad(init_conv)", "nchw_to_nhwc"} <= names
    assert "dense_bwd_x" not in names                       # d(t_emb): x does not reach the conditioning vector
    full = [re.sub(r"<[^>]*>", "", k) for k, _ in forms0]
    assert [re.sub(r"<[^>]*>", "", k) for k, _ in vj].count("gn_bwd") == full.count("gn_bwd")     # the chain itself is all there
    print(f"\n[{cid}] backward plan {count0} entries, data-gradient mode {len(vj)}")
    # without a training forward in the arena the call refuses, as the backward does
    from flocoder_amd.sampling import rk4_time_grid
    model.integrate("rk4", xd.clone(), rk4_time_grid(2), mask=md, mask_is_ones=bool(md is not None and md.min() == 1))
    with pytest.raises(RuntimeError):
        model.vjp_x(xd, td, cd, ed, mask=md)


def test_one_evaluation_at_the_references_stage_states():
    """Interval 0 of the first case: the restatement's four stage states (rounded to fp32) and stage times through a training forward,
    vjp_x(eps) and the stage kernels' reduction.  Both sides see the same x, so the backward's per-sample tolerance covers the whole
    error: |d_gpu - d_64| <= G_TOL |eps_b| |g_j|_b."""
    cid = "d16c10-class"
    sd, x, eps, cond, n, _ = _inputs(cid)
    ref = _ref(cid)
    model = _model(sd)
    ed, cd = eps.to(DEV), cond["class_cond"].to(DEV)
    en = eps.double().flatten(1).norm(dim=1)
    worst = 0.0
    for j, st in enumerate(ref.stages[:4]):
        assert st.interval == 0
        xd = st.x.float().to(DEV)
        td = (torch.full((x.shape[0],), float(st.t), dtype=torch.float32) * 999).to(DEV)
        v = model._forward_native(xd, td, cd, None, train=True)
        g = model.vjp_x(xd, td, cd, ed)
        d = _probe_dot(ed, g).cpu()
        gn = st.g.flatten(1).norm(dim=1)
        ratio = (d - st.d).abs() / (G_TOL * en * gn)
        worst = max(worst, float(ratio.max()))
        print(f"\nstage {j + 1}: d_gpu {d.tolist()}, d_64 {st.d.tolist()}, |d_gpu - d_64| / bound {ratio.tolist()}, "
              f"v rel-L2 {_rel(v, st.v).tolist()}, g rel-L2 {_rel(g, st.g).tolist()}")
        assert bool((ratio <= 1).all()), (j, ratio)
        # (g itself is printed, not gated: G_TOL gates each module's VJP on the GPU's own forward taps, not g end to end.  At time 999
        # the fp32 time sinusoid carries ~6e-5 rad of argument rounding (tests/unet_grad_taps.py), v differs by ~4e-6 and g follows it.)
        # the reduction itself: fp64 products and sums of the GPU's own g, any order
        exact = (eps.double() * g.double().cpu()).flatten(1)
        assert bool(((d - exact.sum(1)).abs() <= 1e-13 * exact.abs().sum(1)).all())
    print(f"worst single-evaluation ratio {worst:.3f}")


@pytest.mark.timeout(900)
@pytest.mark.parametrize("cid", list(CASES))
def test_trajectory_divergence_and_log_likelihood_match_the_fp64_restatement(cid):
    from flocoder_amd import sampling as S
    sd, x, eps, cond, n, reserve = _inputs(cid)
    ref = _ref(cid)
    model = _model(sd, train=False)
    bsz, hw = x.shape[0], x.shape[-1]
    if reserve:
        _reserve_rows(model, reserve, hw)
    xd, ed, cd = x.to(DEV), eps.to(DEV), _dev_cond(cond)
    logp, z, nfe = S.log_likelihood(model, xd, n_steps=n, cond=cd, probe=ed)
    torch.cuda.synchronize()
    assert nfe == 4 * (n - 1) and logp.dtype == torch.float64 and logp.device == xd.device and z.dtype == torch.float32
    assert torch.equal(xd.cpu(), x) and not model.training                      # the input and the model's mode are left alone
    assert all(p.grad is None for p in model.parameters())
    D = x[0].numel()
    a = logp.cpu() + 0.5 * z.double().cpu().flatten(1).pow(2).sum(1) + 0.5 * D * math.log(2 * math.pi)
    # the library's own a (same call through the model method): bit-equal logp, and a as the kernel accumulated it
    z2 = xd.clone()
    mask, ones = S._mask_flags(cd)
    a_k, logp_k = model.log_likelihood(z2, S.rk4_time_grid(n).flip(0), ed, class_ids=None if not cd else cd.get("class_cond"), mask=mask,
                                       mask_is_ones=ones)
    torch.cuda.synchronize()
    z3 = xd.clone()
    a_k2, logp_k2 = model.log_likelihood(z3, S.rk4_time_grid(n).flip(0), ed, class_ids=None if not cd else cd.get("class_cond"), mask=mask,
                                         mask_is_ones=ones)
    torch.cuda.synchronize()
    assert torch.equal(logp_k, logp) and torch.equal(z2, z)                    # calling again gives the same bits: logp, z ...
    assert torch.equal(a_k2, a_k) and torch.equal(logp_k2, logp_k) and torch.equal(z3, z2)      # ... and a
    assert float((a_k.cpu() - a).abs().max()) <= 1e-9 * float(logp.abs().max())
    a = a_k.cpu()
    zr = _rel(z, ref.z)
    bound = lr.a_bound(ref, eps, G_TOL)
    ratio = (a - ref.a).abs() / bound
    lb = bound + 0.5 * (z.double().cpu().flatten(1).pow(2).sum(1) - ref.z.flatten(1).pow(2).sum(1)).abs()
    lratio = (logp.cpu() - ref.logp).abs() / lb
    print(f"\n[{cid}] B={bsz} n={n}: z rel-L2 {zr.tolist()}; a_gpu {a.tolist()}, a_64 {ref.a.tolist()}, bound {bound.tolist()}, "
          f"|a_gpu - a_64| / bound {ratio.tolist()} (worst {float(ratio.max()):.4f}); logp_gpu {logp.tolist()}, logp_64 {ref.logp.tolist()}, "
          f"|logp_gpu - logp_64| / bound {lratio.tolist()}")
    assert torch.isfinite(logp).all() and torch.isfinite(z).all()
    assert float(zr.max()) < TRAJ_TOL, zr
    assert bool((ratio <= 1).all()), ratio
    assert bool((lratio <= 1).all()), lratio

    # inversion: the captured inference path on the reversed grid, against the reversed RK4 of the restatement and against z above
    zi, nfe_i = S.invert_latents(model, xd, n_steps=n, cond=cd)
    torch.cuda.synchronize()
    assert nfe_i == nfe and torch.equal(xd.cpu(), x)
    sd64 = {k: v.double() for k, v in sd.items()}
    zi_ref = lr.invert_ref(sd64, x.double(), n, cond)
    print(f"  invert_latents rel-L2 {_rel(zi, zi_ref).tolist()}, against log_likelihood's z {_rel(zi, z).tolist()}")
    assert float(_rel(zi, zi_ref).max()) < TRAJ_TOL and float(_rel(zi, z).max()) < TRAJ_TOL
    assert float(_rel(zi_ref, ref.z).max()) <= 1e-12                            # (the restatement's two forms agree)


def test_guidance_and_bad_arguments_are_refused_on_the_gpu():
    from flocoder_amd import sampling as S
    sd, x, eps, cond, n, _ = _inputs("d16c10-class")
    model = _model(sd, train=False)
    xd, cd = x.to(DEV), _dev_cond(cond)
    with pytest.raises(ValueError, match="guidance"):
        S.log_likelihood(model, xd, n_steps=n, cond=cd, cfg_strength=3.0)
    with pytest.raises(ValueError, match="shape"):
        S.log_likelihood(model, xd, n_steps=n, cond=cd, probe=torch.ones(3, 4, 16, 8, device=DEV))
    with pytest.raises(IndexError):
        S.log_likelihood(model, xd, n_steps=n, cond={"class_cond": torch.tensor([0, 1, 10], device=DEV)})
    with pytest.raises(ValueError):
        model.log_likelihood(xd.clone(), S.rk4_time_grid(1), eps.to(DEV))
    lp, _, _ = S.log_likelihood(model, xd, n_steps=3, cond=cd, generator=torch.Generator(device=DEV).manual_seed(1))
    lq, _, _ = S.log_likelihood(model, xd, n_steps=3, cond=cd, generator=torch.Generator(device=DEV).manual_seed(1))
    assert torch.equal(lp, lq) and torch.isfinite(lp).all()


@pytest.mark.timeout(600)
def test_a_likelihood_call_leaks_nothing_into_training_or_sampling():
    """A log_likelihood call between two FlowTrainer steps leaves the second step's loss and gradients bit-equal to a run without it (the
    call moves the arena serial; the step runs its own forward anyway), and the parameters after it too.  A sampler call right after a
    likelihood call equals, in bits, the same call on a fresh model: the likelihood needs the training form of the handle's plans and
    puts the inference form back when it was the one that switched (Unet.log_likelihood, restore_plan)."""
    from flocoder_amd import sampling as S
    from flocoder_amd.train import FlowTrainer
    g = load_golden("g10_train_step")
    sd = synth_state_dict(g["shapes"], 10)
    cls = torch.from_numpy(g["cls"]).to(DEV)
    xl, el = synth_input("ll.hyg.x", (8, 4, 16, 16), 1).to(DEV), torch.where(synth_input("ll.hyg.e", (8, 4, 16, 16), 1) >= 0, 1.0, -1.0).to(DEV)

    def run(with_ll):
        from flocoder_amd.unet import Unet
        m = Unet(dim=16, channels=4, dim_mults=(1, 2, 4, 8), n_classes=10)
        m.load_state_dict(sd)
        tr = FlowTrainer(m.to(DEV).train(), lr=1e-4)
        out = []
        for step in (1, 2):
            src, tgt = synth_input(f"g10.src{step}", (8, 4, 16, 16), 10), synth_input(f"g10.tgt{step}", (8, 4, 16, 16), 10)
            u = torch.sigmoid(synth_input(f"g10.u{step}", (8,), 10, scale=1.5))
            loss = tr.step(src.to(DEV), tgt.to(DEV), {"class_cond": cls, "mask_cond": None}, u=u.to(DEV))
            out.append((loss.clone(), tr.grads.clone(), tr.params.clone()))
            if with_ll and step == 1:
                serial = m.arena_serial()
                lp, _, _ = S.log_likelihood(m, xl, n_steps=3, cond={"class_cond": cls}, probe=el)
                assert m.arena_serial() != serial and m.training and torch.isfinite(lp).all()
        torch.cuda.synchronize()
        return out

    plain, mixed = run(False), run(True)
    for (l0, g0, p0), (l1, g1, p1) in zip(plain, mixed):
        assert torch.equal(l0, l1) and torch.equal(g0, g1) and torch.equal(p0, p1)

    src = synth_input("ll.hyg.src", (8, 4, 16, 16), 2).to(DEV)
    cond = {"class_cond": cls}
    from flocoder_amd import _binding as B
    used, fresh = _model(sd, train=False), _model(sd, train=False)
    lp1, _, _ = S.log_likelihood(used, xl, n_steps=3, cond=cond, probe=el)
    lp2, _, _ = S.log_likelihood(used, xl, n_steps=3, cond=cond, probe=el)
    assert torch.equal(lp1, lp2)
    assert B.lib().fc_unet_train_form(used._handle) == 0                        # the handle is back in the inference form
    lat_u, _ = S.generate_latents_rk4(used, (8, 4, 16, 16), 4, cond, 3.0, source=src)
    lat_f, _ = S.generate_latents_rk4(fresh, (8, 4, 16, 16), 4, cond, 3.0, source=src)
    torch.cuda.synchronize()
    assert torch.equal(lat_u, lat_f)
    assert used.launches_per_forward == fresh.launches_per_forward
    # a reservation the caller made before the call is there again after it, in the form it had
    used.reserve(24, 16, 16)
    n_inf = used.launches_per_forward
    S.log_likelihood(used, xl, n_steps=3, cond=cond, probe=el)
    assert used.chains[1] == 24 and used.launches_per_forward == n_inf and B.lib().fc_unet_train_form(used._handle) == 0
    # restore_plan=False keeps the training form until release_training_plan()
    a1, l1 = used.log_likelihood(xl.clone(), S.rk4_time_grid(3).flip(0), el, class_ids=cls, restore_plan=False)
    assert B.lib().fc_unet_train_form(used._handle) == 1
    a2, l2 = used.log_likelihood(xl.clone(), S.rk4_time_grid(3).flip(0), el, class_ids=cls, restore_plan=False)
    assert torch.equal(a1, a2) and torch.equal(l1, l2)
    used.release_training_plan()
    assert B.lib().fc_unet_train_form(used._handle) == 0
    # a probe that is a view at an odd storage offset is accepted (copied to an aligned buffer), with the same result
    odd = torch.empty(el.numel() + 1, device=DEV)[1:].view_as(el).copy_(el)
    lp_odd, _, _ = S.log_likelihood(_model(sd, train=False), xl, n_steps=3, cond=cond, probe=odd)
    torch.cuda.synchronize()
    assert odd.data_ptr() % 16 != 0 and torch.equal(lp_odd, lp1)
