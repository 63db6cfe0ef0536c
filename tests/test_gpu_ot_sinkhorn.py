"""The entropic OT plan on the device (fc_ot_sinkhorn, fc_ot_plan_sinkhorn), plan sampling (fc_ot_sample_plan) and the plan as a
permutation (fc_ot_plan_pairing) against tests/ot_sinkhorn_ref.py.

The certificate, on the device's own outputs, in fp64 on the host (ot_sinkhorn_ref.certificate):
 (a) every plan entry equals exp((f_i + g_j - C_ij)/reg) of the returned duals and cost within 2^-23 relative, or is below fp32's smallest
     normal -- fp32 storage (2^-24) is the only rounding of that size, the device's and the host's fp64 exp differ by a few 2^-53;
 (b) |colsum - 1/B|_2 of that Gibbs form is <= stop_thr + 1e-12 when `converged` is set, and equals the reported err within 1e-12
     (fp64 sums of <= 1024 terms of magnitude <= 1 are good to ~1e-13);
 (c) its row sums are within 1e-12 of 1/B (the row half comes last; the potentials' own rounding, 2^-53 |f| / reg, is ~1e-14);
 (d) <P, C> lies between the assignment optimum / B and mean(C), with slack sqrt(B) err max(C) for the marginals' error.
A Gibbs-form matrix with these marginals is the entropic optimum of the (slightly perturbed) marginals, so (a)-(c) are complete.
(b) and (c) are taken on the Gibbs form, not on the stored fp32 entries: those carry 2^-24 each, which is what (a) bounds.

The iteration count and the converged flag must equal the restatement's on the device's cost matrix: tests/test_ot_sinkhorn_cpu.py
shows no stopping check within 1 % of stop_thr on these cases."""
import functools

import numpy as np
import pytest
import torch

import ot_sinkhorn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _device_run(case):
    """compute_ot_plan on the case's points -> host copies of everything it returned (one run per session)."""
    from flocoder_amd.ot import compute_ot_plan
    B, D, reg, normalised, max_iter = case
    s, t = R.points(B, D)
    plan, info = compute_ot_plan(_dev(s), _dev(t), reg=reg, normalize_cost=normalised, max_iter=max_iter, stop_thr=R.STOP_THR, return_info=True)
    assert plan.dtype == torch.float32 and plan.shape == (B, B) and plan.device.type == "cuda"
    assert info["f"].dtype == torch.float64 and info["iterations"].dtype == torch.int64 and info["converged"].dtype == torch.bool
    assert all(v.device.type == "cuda" for v in info.values())
    return plan.cpu().numpy(), {k: v.cpu().numpy() for k, v in info.items()}


def _certify(plan, cost, f, g, reg, err, conv, tag):
    B = cost.shape[0]
    cert = R.certificate(plan, cost, f, g, reg)
    print(f"{tag}: form {cert['form']:.3e} (2^-23 = {2.0 ** -23:.3e}), col {cert['col']:.3e} (reported {err:.3e}), row {cert['row']:.3e}")
    assert np.isfinite(plan).all() and np.isfinite(f).all() and np.isfinite(g).all()
    assert cert["form"] <= 2.0 ** -23 and cert["small_ok"], tag                                        # (a)
    assert abs(cert["col"] - err) <= 1e-12, tag                                                        # (b)
    if conv:
        assert cert["col"] <= R.STOP_THR + 1e-12, tag
    assert cert["row"] <= 1e-12, tag                                                                   # (c)
    lo, hi = R.cost_bounds(cost)                                                                       # (d)
    slack = np.sqrt(B) * err * float(cost.max())
    print(f"{tag}: <P, C> = {cert['cost']:.6f} in [{lo:.6f}, {hi:.6f}], slack {slack:.2e}")
    assert lo - slack <= cert["cost"] <= hi + slack, tag


@pytest.mark.parametrize("case", R.CASES)
def test_plan_meets_the_certificate_and_stops_where_the_restatement_does(case):
    B, D, reg, normalised, max_iter = case
    plan, info = _device_run(case)
    cost, f, g = info["cost"], info["f"], info["g"]
    ref = R.host_cost(B, D, normalised)
    dc = float(np.abs(cost.astype(np.float64) - ref).max() / max(float(ref.max()), 1e-30))
    print(f"{case}: device cost against the host's, max difference / max {dc:.2e}")
    assert dc < 1e-5 and (not normalised or B == 1 or float(cost.max()) == 1.0)
    it, conv, err = int(info["iterations"]), bool(info["converged"]), float(info["err"])
    _certify(plan, cost, f, g, reg, err, conv, str(case))
    _, rf, rg, rit, rconv, rerr = R.sinkhorn(cost, reg, max_iter, R.STOP_THR)
    shift = float(np.mean(f - rf))
    print(f"{case}: {it} iterations (restatement {rit}), err {err:.3e} ({rerr:.3e}), potentials differ by "
          f"{max(np.abs(f - rf - shift).max(), np.abs(g - rg + shift).max()) / reg:.2e} reg (free constant {shift / reg:.1e} reg)")
    assert (it, conv) == (rit, rconv)


@pytest.mark.parametrize("case", R.STUCK_CASES)
def test_no_convergence_is_reported_and_the_outputs_stay_finite(case):
    B, D, reg, normalised, max_iter = case
    plan, info = _device_run(case)
    it, conv, err = int(info["iterations"]), bool(info["converged"]), float(info["err"])
    print(f"{case}: {it} iterations, converged {conv}, err {err:.3e}")
    assert it == max_iter and not conv and err >= R.STOP_THR
    _certify(plan, info["cost"], info["f"], info["g"], reg, err, conv, str(case))


def test_solver_alone_hazards_and_arguments():
    from flocoder_amd import _binding as Bn
    from flocoder_amd._ops import ot_sinkhorn
    from flocoder_amd.ot import compute_ot_plan
    for B in (64, 70):                                    # all-equal costs: the uniform plan, exactly
        plan, duals, info = ot_sinkhorn(_dev(R.equal_matrix(B)), 0.05)
        assert info.cpu().tolist()[:2] == [10.0, 1.0] and float(info[2]) < 1e-15
        assert np.array_equal(plan.cpu().numpy(), np.full((B, B), np.float32(1.0 / (B * B)))), B
    raw = R.host_cost(70, 32, True).copy()                # a non-finite row, a lone non-finite entry
    raw[5] = np.nan
    raw[9, 3] = np.inf
    plan, duals, info = ot_sinkhorn(_dev(raw), 0.05, max_iter=50)
    p, d = plan.cpu().numpy(), duals.cpu().numpy()
    assert np.isfinite(p).all() and np.isfinite(d).all() and np.isfinite(info.cpu().numpy()).all()
    assert p[9, 3] == 0.0 and (p[5] <= np.float32(1.0 / 70)).all() and abs(float(p[np.arange(70) != 5].sum(1).max()) - 1 / 70) < 1e-7
    # a non-finite COLUMN (a non-finite target sample), alone and with the row: its entries are exp(f_i / reg) <= 1/B, not ones; the
    # rows' sums include them (the row half comes last); the solver still converges, every other line's marginal being enforced
    for rows in ((), (5,)):
        raw = R.host_cost(70, 32, True).copy()
        raw[:, 40] = np.inf
        for r in rows:
            raw[r] = np.nan
        plan, duals, info = ot_sinkhorn(_dev(raw), 0.05)
        p, d, nf_ = plan.cpu().numpy().astype(np.float64), duals.cpu().numpy(), info.cpu().numpy()
        keep = np.array([i not in rows for i in range(70)])
        print(f"sentinel column, sentinel rows {rows}: {nf_[0]:.0f} iterations, converged {nf_[1]:.0f}, err {nf_[2]:.2e}, plan sum {p.sum():.9f}, "
              f"column sum {p[:, 40].sum():.6f}")
        assert np.isfinite(p).all() and np.isfinite(d).all() and np.isfinite(nf_).all()
        assert (p[:, 40] <= np.float32(1.0 / 70)).all() and np.abs(p[keep].sum(1) - 1 / 70).max() < 1e-7
        assert np.abs(np.delete(p, 40, 1).sum(0) - 1 / 70).max() < 1e-7 + nf_[2] and abs(p.sum() - 1.0) < 1e-5 + 70 * nf_[2]
    s, t = R.points(70, 32)
    s[5] = np.nan
    plan, inf2 = compute_ot_plan(_dev(s), _dev(t), normalize_cost=True, return_info=True)
    c = inf2["cost"].cpu().numpy()
    assert np.isfinite(plan.cpu().numpy()).all() and (c[5] == np.float32(R.X.FLT_MAX)).all() and float(np.delete(c, 5, 0).max()) == 1.0
    # max_iter is rounded up to the check period
    assert float(ot_sinkhorn(_dev(R.host_cost(7, 16, True)), 0.05, max_iter=11, stop_thr=0.0)[2][0]) == 20.0
    z, st = torch.zeros(8, 8, device=DEV), Bn.current_stream(torch.device(DEV))
    pl, du, nf = torch.zeros(8, 8, device=DEV), torch.zeros(16, device=DEV, dtype=torch.float64), torch.zeros(3, device=DEV, dtype=torch.float64)
    call = lambda c_, b_, reg, mi, thr: Bn.lib().fc_ot_sinkhorn(c_, b_, reg, mi, thr, Bn.ptr(pl), Bn.ptr(du), Bn.ptr(nf), st)
    assert call(Bn.ptr(z), 0, 0.05, 10, 1e-9) == Bn.FC_E_SHAPE and call(Bn.ptr(z), 1025, 0.05, 10, 1e-9) == Bn.FC_E_SHAPE
    assert call(None, 8, 0.05, 10, 1e-9) == Bn.FC_E_ARG and call(Bn.ptr(z), 8, 0.0, 10, 1e-9) == Bn.FC_E_ARG
    assert call(Bn.ptr(z), 8, float("nan"), 10, 1e-9) == Bn.FC_E_ARG and call(Bn.ptr(z), 8, 0.05, 10, -1.0) == Bn.FC_E_ARG
    assert call(Bn.ptr(z), 8, 0.05, 0, 1e-9) == Bn.FC_E_ARG and call(Bn.ptr(z), 8, 0.05, 10001, 1e-9) == Bn.FC_E_ARG
    assert Bn.lib().fc_ot_plan_sinkhorn(Bn.ptr(z), Bn.ptr(z), 8, 8, 0.05, 0, 10, 1e-9, Bn.ptr(pl), Bn.ptr(du), Bn.ptr(nf), None, st) == Bn.FC_E_ARG
    assert Bn.lib().fc_ot_sample_plan(Bn.ptr(pl), 8, 0, 0, 0, Bn.ptr(du), Bn.ptr(du), None, st) == Bn.FC_E_SHAPE
    assert Bn.lib().fc_ot_sample_plan(Bn.ptr(pl), 8, 65537, 0, 0, Bn.ptr(du), Bn.ptr(du), None, st) == Bn.FC_E_SHAPE
    assert Bn.lib().fc_ot_plan_pairing(None, 8, Bn.ptr(du), st) == Bn.FC_E_ARG
    for bad in (dict(reg=0.0), dict(max_iter=0), dict(stop_thr=-1.0)):
        with pytest.raises(ValueError):
            compute_ot_plan(z, z, **bad)
    with pytest.raises(ValueError):
        compute_ot_plan(torch.zeros(1025, 2, device=DEV), torch.zeros(1025, 2, device=DEV))


@pytest.mark.parametrize("B,D,reg", R.SAMPLE_CASES[:3])
def test_sampled_pairs_are_the_restatements_bits(B, D, reg):
    from flocoder_amd.noise import plan_uniforms
    from flocoder_amd.ot import sample_plan
    plan = _device_run((B, D, reg, True, 1000))[0]
    pd = _dev(plan)
    seen = {}
    for seed, draw in ((12345, 0), (2 ** 63 + 5, 7)):
        for n in (1, B, 4096):
            i, j = sample_plan(pd, n, seed=seed, draw_index=draw)
            assert i.dtype == torch.int64 and i.shape == (n,)
            ri, rj, ok = R.sample_two_level(plan, plan_uniforms(seed, draw, n))
            assert ok and np.array_equal(i.cpu().numpy(), ri) and np.array_equal(j.cpu().numpy(), rj), (seed, draw, n)
            seen[(seed, draw, n)] = (i, j)
    i2, j2 = sample_plan(pd, 4096, seed=12345, draw_index=0)
    assert torch.equal(i2, seen[(12345, 0, 4096)][0]) and torch.equal(j2, seen[(12345, 0, 4096)][1])
    i3, j3 = sample_plan(pd, 4096, seed=12345, draw_index=1)
    assert B == 1 or not (torch.equal(i3, i2) and torch.equal(j3, j2))
    assert torch.equal(sample_plan(pd)[0], sample_plan(pd, B)[0])                     # the default count is the batch


def test_sampling_a_degenerate_plan_gives_identity_pairs_and_a_sticky_flag():
    from flocoder_amd._ops import ot_sample_plan
    flag = torch.zeros(1, device=DEV, dtype=torch.int32)
    good = _dev(_device_run((7, 16, 0.05, True, 1000))[0])
    ot_sample_plan(good, 9, info=flag)
    assert int(flag) == 0
    for bad in (torch.zeros(7, 7, device=DEV), torch.full((7, 7), float("nan"), device=DEV)):
        i, j = ot_sample_plan(bad, 9, info=flag)
        assert i.tolist() == [0, 1, 2, 3, 4, 5, 6, 0, 1] and torch.equal(i, j) and int(flag) == 1
    ot_sample_plan(good, 9, info=flag)
    assert int(flag) == 1                                                            # sticky


def test_plan_pairing_is_the_restatements_sweep():
    from flocoder_amd._ops import ot_plan_pairing
    from flocoder_amd.ot import compute_ot_pairing, pairing_cost
    for case in ((7, 16, 0.05, True, 1000), (65, 32, 0.05, True, 1000), (193, 16, 0.05, True, 1000)):
        plan = _device_run(case)[0]
        perm = ot_plan_pairing(_dev(plan)).cpu().numpy()
        assert R.X.is_permutation(perm, case[0]) and np.array_equal(perm, R.plan_pairing(plan))
    assert np.array_equal(ot_plan_pairing(_dev(np.full((70, 70), 0.25, np.float32))).cpu().numpy(), np.arange(70))
    s, t = (_dev(a) for a in R.points(64, 1024))
    perm = compute_ot_pairing(s, t, method="sinkhorn")
    assert perm.dtype == torch.int64 and R.X.is_permutation(perm.cpu().numpy(), 64)
    cs, ci = float(pairing_cost(s, t, perm)), float(pairing_cost(s, t))
    print(f"(64, 1024): pairing cost identity {ci:.4f}, sinkhorn {cs:.4f}")
    assert cs <= ci


def test_greedy_and_exact_bits_stay_around_a_sinkhorn_call():
    from flocoder_amd._ops import ot_pairing, ot_pairing_exact, ot_plan_sinkhorn
    s, t = (_dev(a) for a in R.points(130, 37))
    g0, e0 = ot_pairing(s, t), ot_pairing_exact(s, t)
    a, b = ot_plan_sinkhorn(s, t, 0.05, True), ot_plan_sinkhorn(s, t, 0.05, True)     # back to back on one stream
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    g1, e1 = ot_pairing(s, t), ot_pairing_exact(s, t)
    for x, y in zip(g0 + e0, g1 + e1):
        assert torch.equal(x, y)


# ---- the sampler object and the training path -----------------------------------------------------------------------------------
def test_ot_plan_sampler_surface():
    from flocoder_amd import OTPlanSampler
    from flocoder_amd.ot import compute_ot_pairing_exact, compute_ot_plan, sample_plan
    s, t = (_dev(a) for a in R.points(65, 32))
    y0, y1 = torch.arange(65, device=DEV), torch.arange(65, device=DEV) + 100
    sk = OTPlanSampler("sinkhorn", reg=0.05, normalize_cost=True, seed=3)
    pi = sk.get_map(s, t)
    assert torch.equal(pi, compute_ot_plan(s, t, reg=0.05, normalize_cost=True))
    i, j = sample_plan(pi, 65, seed=3, draw_index=0)
    x0, x1 = sk.sample_plan(s, t)
    assert torch.equal(x0, s[i]) and torch.equal(x1, t[j]) and sk.draw_index == 1
    x0, x1, l0, l1 = sk.sample_plan_with_labels(s, t, y0, y1)
    i, j = sample_plan(pi, 65, seed=3, draw_index=1)
    assert torch.equal(x0, s[i]) and torch.equal(x1, t[j]) and torch.equal(l0, y0[i]) and torch.equal(l1, y1[j]) and sk.draw_index == 2
    assert sk.sample_plan_with_labels(s, t)[2:] == (None, None)
    resumed = OTPlanSampler("sinkhorn", reg=0.05, normalize_cost=True)
    resumed.load_state_dict({"seed": 3, "draw_index": 1})
    assert torch.equal(resumed.sample_map(pi, 65)[0], i)
    ex = OTPlanSampler("exact")
    pe = ex.get_map(s, t)
    perm = compute_ot_pairing_exact(s, t)
    assert float(pe.sum()) == pytest.approx(1.0, abs=1e-6) and torch.equal(pe.argmax(1), perm) and int((pe > 0).sum()) == 65
    i, j = ex.sample_map(pe, 300)
    assert torch.equal(j, perm[i])                                                   # a permutation plan only ever pairs i with perm[i]


def _trainer(seed=0):
    from flocoder_amd.train import FlowTrainer
    from flocoder_amd.unet import Unet
    torch.manual_seed(seed)
    return FlowTrainer(Unet(dim=32, channels=4, dim_mults=(1, 2, 4, 8), n_classes=10).to(DEV).train(), lr=1e-3)


def _batch():
    g = torch.Generator().manual_seed(5)
    return torch.randn(16, 4, 8, 8, generator=g), torch.randn(16, 4, 8, 8, generator=g) * 0.7, torch.randint(0, 10, (16,), generator=g)


def test_step_takes_a_pairing_with_repeats():
    src, tgt, cls = (x.to(DEV) for x in _batch())
    u = torch.rand(16, generator=torch.Generator().manual_seed(6)).to(DEV)
    j = torch.tensor([3, 3, 0, 15, 7, 7, 7, 1, 2, 2, 9, 9, 14, 0, 3, 5], device=DEV)
    a, b = _trainer(), _trainer()
    la = a.step(src, tgt, {"class_cond": cls}, u=u, pairing=j)
    lb = b.step(src, tgt[j].contiguous(), {"class_cond": cls}, u=u)
    assert float(la) == float(lb) and torch.equal(a.params, b.params)


def test_training_path_takes_the_sinkhorn_methods():
    from flocoder_amd.ot import compute_ot_pairing, compute_ot_plan, sample_plan
    from flocoder_amd.train import batch_to_data
    _, lat, cls = _batch()
    target = lat.to(DEV)
    torch.manual_seed(3)
    src, tgt, _, _, _ = batch_to_data((lat, cls), torch.device(DEV), ot_method="sinkhorn")
    torch.manual_seed(3)
    noise = torch.randn_like(target)
    assert torch.equal(src, noise) and torch.equal(tgt, target[compute_ot_pairing(noise, target, method="sinkhorn")])
    torch.manual_seed(3)
    src, tgt, c2, _, _ = batch_to_data((lat, cls), torch.device(DEV), ot_method="sinkhorn_sample", ot_draw=(11, 4))
    i, j = sample_plan(compute_ot_plan(noise, target, reg=0.05, normalize_cost=True), seed=11, draw_index=4)
    assert torch.equal(src, noise[i]) and torch.equal(tgt, target[j]) and torch.equal(c2, cls.to(DEV)[j])
    # train_batch: "sinkhorn" is step fed that pairing; "sinkhorn_sample" is step on the drawn rows, counts its draws and moves the loss
    a, b = _trainer(1), _trainer(1)
    torch.manual_seed(4)
    la = a.train_batch((lat, cls), cfg_drop=0.0, ot_method="sinkhorn")
    torch.manual_seed(4)
    noise = torch.randn_like(target)
    lb = b.step(noise, target[compute_ot_pairing(noise, target, method="sinkhorn")], {"class_cond": cls.to(DEV), "mask_cond": None})
    assert float(la) == float(lb) and torch.equal(a.params, b.params)
    tr, ref = _trainer(2), _trainer(2)
    p0 = tr.params.clone()
    torch.manual_seed(4)
    first = float(tr.train_batch((lat, cls), cfg_drop=0.0, ot_method="sinkhorn_sample"))
    assert tr.ot_draws == 1 and np.isfinite(first) and not torch.equal(tr.params, p0)
    torch.manual_seed(4)
    noise = torch.randn_like(target)
    i, j = sample_plan(compute_ot_plan(noise, target, reg=0.05, normalize_cost=True), seed=0, draw_index=0)
    assert float(ref.step(noise[i], target[j], {"class_cond": cls.to(DEV)[j], "mask_cond": None})) == first and torch.equal(ref.params, tr.params)
    losses = [first] + [float(tr.train_batch((lat, cls), cfg_drop=0.0, ot_method="sinkhorn_sample")) for _ in range(3)]
    print("sinkhorn_sample losses:", " ".join(f"{x:.4f}" for x in losses))
    assert tr.ot_draws == 4 and all(np.isfinite(losses)) and len(set(losses)) == 4        # every batch is another draw: the loss moves
    batch = ({"target_latents": lat, "source_latents": lat, "mask_pixels": torch.zeros(16, 1, 128, 128)}, cls)
    with pytest.raises(ValueError):
        tr.train_batch(batch, ot_method="sinkhorn_sample")


def test_trainer_state_carries_the_draw_counter_and_ot_reg_reaches_the_solver():
    from flocoder_amd.ot import compute_ot_pairing
    from flocoder_amd.train import batch_to_data
    _, lat, cls = _batch()
    tr = _trainer(3)
    tr.ot_seed = 21
    for _ in range(2):
        tr.train_batch((lat, cls), cfg_drop=0.0, ot_method="sinkhorn_sample", ot_reg=0.1)
    sd = tr.state_dict()
    assert sd["ot_seed"] == 21 and sd["ot_draws"] == 2
    other = _trainer(3)
    other.load_state_dict(sd)
    assert (other.ot_seed, other.ot_draws) == (21, 2)
    old = {k: v for k, v in sd.items() if not k.startswith("ot_")}                   # a checkpoint from before the counter existed
    other.load_state_dict(old)
    assert (other.ot_seed, other.ot_draws) == (0, 0)
    target = lat.to(DEV)
    torch.manual_seed(3)
    _, tgt, _, _, _ = batch_to_data((lat, cls), torch.device(DEV), ot_method="sinkhorn", ot_reg=0.02)
    torch.manual_seed(3)
    noise = torch.randn_like(target)
    assert torch.equal(tgt, target[compute_ot_pairing(noise, target, method="sinkhorn", reg=0.02)])


def test_inpaint_step_takes_the_sinkhorn_pairing():
    """inpaint_step(ot=True, ot_method="sinkhorn") is inpaint_step on the target gathered by that pairing of the blended source."""
    from flocoder_amd.inpainting import MaskEncoder, mask_blending
    from flocoder_amd.ot import compute_ot_pairing
    from flocoder_amd.train import FlowTrainer
    from flocoder_amd.unet import Unet

    def make():
        torch.manual_seed(31)
        model, me = Unet(dim=8, channels=4, dim_mults=(1, 2, 4, 8), n_classes=0, mask_cond=True).to(DEV).train(), MaskEncoder().to(DEV).train()
        tr = FlowTrainer(model, lr=1e-3)
        tr.attach_mask_encoder(me)
        return tr
    a, b = make(), make()
    gen = torch.Generator().manual_seed(32)
    tgt, s0, noise = (torch.randn(6, 4, 8, 8, generator=gen).to(DEV) for _ in range(3))
    pix = (torch.rand(6, 1, 128, 128, generator=gen) > 0.5).float().to(DEV)
    u = torch.rand(6, generator=gen).to(DEV)
    with torch.no_grad():
        source = mask_blending(s0, b.me._forward_native(pix), noise)
    perm = compute_ot_pairing(source, tgt, method="sinkhorn")
    assert R.X.is_permutation(perm.cpu().numpy(), 6)
    la = a.inpaint_step(s0, tgt, pix, noise=noise, u=u, ot=True, ot_method="sinkhorn")
    lb = b.inpaint_step(s0, tgt[perm].contiguous(), pix, noise=noise, u=u)
    assert torch.equal(la, lb) and torch.equal(a.params, b.params) and torch.equal(a.me_params, b.me_params)
