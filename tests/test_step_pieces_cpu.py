"""tests/step_pieces_ref.py held to torch itself, and its bounds held to what fp32 can deliver (no GPU).

  * the fp64 references equal ``torch.optim.Adam``, ``clip_grad_norm_``, ``nn.MSELoss`` and the prologue lines of train_flow.py:350-355
    run in float64;
  * on every input set tests/test_gpu_step_pieces.py uses, torch's own fp32 evaluation -- and for the two reductions an fp32 emulation
    of the kernels' partition (256 x 256 grid-stride threads, then the two block_sum trees) -- stays inside each bound.  That is what
    keeps the GPU gates honest: a bound that correct fp32 arithmetic could miss would be a wrong bound.  Worst ratios are printed.
"""
import math

import pytest
import torch

import step_pieces_ref as R
from flocoder_amd.sampling import warp_time

F32, F64 = torch.float32, torch.float64


def _close64(a, b, what):
    assert torch.allclose(a, b, rtol=1e-13, atol=0), (what, float((a - b).abs().max()))


# ---- the references are torch's own operations in float64 -----------------------------------------------------------------------------
@pytest.mark.parametrize("state,step", R.ADAM_STATES)
@pytest.mark.parametrize("coef", R.ADAM_COEF)
def test_adam_reference_is_torch_optim_adam_in_float64(state, step, coef):
    p, g, m, v, ema = R.adam_inputs(4099, state, 1e-4, seed=11 + step)
    lr = 1e-3
    ref = R.adam_ema(p, g, m, v, ema, coef, lr, R.B1, R.B2, R.EPS, step, R.DECAY)
    w = torch.nn.Parameter(p.to(F64).clone())
    opt = torch.optim.Adam([w], lr=lr, betas=(R.B1, R.B2), eps=R.EPS, foreach=False)
    opt.state[w] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.to(F64).clone(), "exp_avg_sq": v.to(F64).clone()}
    w.grad = R.clipped(g, coef).to(F64)                  # what clip_grad_norm_ leaves in p.grad
    opt.step()
    _close64(w.detach(), ref[0], "p")
    _close64(opt.state[w]["exp_avg"], ref[1], "exp_avg")
    _close64(opt.state[w]["exp_avg_sq"], ref[2], "exp_avg_sq")
    assert int(opt.state[w]["step"]) == step
    _close64(R.DECAY * ema.to(F64) + (1.0 - R.DECAY) * w.detach(), ref[3], "ema")          # train_flow.py:46-54
    skip = R.adam_ema(p, g, m, v, ema, coef, lr, R.B1, R.B2, R.EPS, step, R.DECAY, apply_adam=False)
    assert torch.equal(skip[0], p.to(F64)) and torch.equal(skip[1], m.to(F64)) and torch.equal(skip[2], v.to(F64))
    _close64(R.DECAY * ema.to(F64) + (1.0 - R.DECAY) * p.to(F64), skip[3], "ema without a gradient")


def test_clip_reference_is_clip_grad_norm_in_float64():
    for name, g, g2, max_norm in R.clip_cases():
        ps = [torch.nn.Parameter(torch.zeros(t.numel(), dtype=F64)) for t in (g, g2) if t is not None]
        for q, t in zip(ps, (g, g2)):
            q.grad = t.to(F64).clone()
        total = torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)
        norm, coef = R.clip(g, g2, max_norm)
        _close64(total, norm, name)
        _close64(ps[0].grad, g.to(F64) * coef, name)
        if name == "zeros":
            assert float(norm) == 0.0 and float(coef) == 1.0
        else:
            assert (float(coef) == 1.0) == ("x0.5" in name), name


def test_mse_reference_is_mseloss_in_float64():
    for name, v, tgt in R.loss_cases():
        vv = v.to(F64).clone().requires_grad_(True)
        loss = torch.nn.MSELoss()(vv, tgt.to(F64))
        loss.backward()
        ref_loss, ref_dv = R.mse(v, tgt)
        _close64(loss.detach(), ref_loss, name)
        _close64(vv.grad, ref_dv, name)


def test_prepare_reference_is_the_prologue_of_the_training_loop_in_float64():
    for c in R.prologue_cases():
        if c["pairing"] is not None and bool(((c["pairing"] < 0) | (c["pairing"] >= c["target_rows"])).any()):
            continue                                               # target[ot_indices] raises upstream: the fallback is ours, checked below
        ref = R.prepare(c["src"], c["tgt"], c["u"], R.T_EPS, c["warp_s"], R.T_SCALE, c["pairing"], c["ids"], R.N_CLASSES, c["first_row"],
                        c["target_rows"])
        source, target = c["src"].to(F64), c["tgt"].to(F64)
        lo = c["first_row"]
        target = target[c["pairing"]] if c["pairing"] is not None else target[lo:lo + c["batch"]]
        t = warp_time(c["u"].to(F64) * (1 - R.T_EPS) + R.T_EPS, s=c["warp_s"])                      # train_flow.py:350-351
        t_expand = t.view(-1, 1).repeat(1, target.shape[1])
        _close64(t, ref["t"], c["name"])
        _close64(t * 999, ref["time"], c["name"])
        assert torch.allclose((1 - t_expand) * source + t_expand * target, ref["x"], rtol=1e-13, atol=1e-15), c["name"]
        assert torch.equal(target - source, ref["v"]), c["name"]


def test_prepare_reference_flags_and_fallback_rows():
    seen = set()
    for c in R.prologue_cases():
        ref = R.prepare(c["src"], c["tgt"], c["u"], R.T_EPS, c["warp_s"], R.T_SCALE, c["pairing"], c["ids"], R.N_CLASSES, c["first_row"],
                        c["target_rows"])
        name = c["name"]
        assert bool(ref["flag"] & 2) == ("-bad-" in name), name
        assert bool(ref["flag"] & 1) == any(k in name for k in ("-high-", "-neg-", "-bad_noflag-")), name
        if "-bad-" in name:
            bad = (c["pairing"] < 0) | (c["pairing"] >= c["target_rows"])
            own = c["first_row"] + torch.arange(c["batch"])
            assert torch.equal(ref["rows"][bad], own[bad]) and torch.equal(ref["rows"][~bad], c["pairing"][~bad])
            seen.update(int(e) == -1 and "low" or "high" for e in c["pairing"][bad])
        assert float(c["u"].min()) == 0.0 or float(c["u"].max()) == 1.0
    assert seen == {"low", "high"}
    names = " ".join(c["name"] for c in R.prologue_cases())
    for s in R.WARP_S:
        assert f"-s{s}-" in names
    for k in ("-none-", "-perm-", "-repeats-", "-bad-", "-ok-", "-high-", "-neg-", "-bad_noflag-", "-rows", "-plain"):
        assert k in names, k


# ---- the bounds hold for correct fp32 arithmetic --------------------------------------------------------------------------------------
def _report(worst, info=None):
    """``info``: torch's own fp32 sums, printed and not asserted -- their order is torch's (long per-lane chains on the CPU), not the
    partition the reduction bounds count."""
    for k, r in {**worst, **(info or {})}.items():
        print(f"worst ratio of fp32 error to bound, {k}: {r:.3f}")
    for k, r in worst.items():
        assert r < 1.0, (k, r)


def test_prologue_bounds_hold_for_torch_fp32():
    worst = {"t": 0.0, "x": 0.0, "x (interp)": 0.0}
    for c in R.prologue_cases():
        s32, g32 = c["src"], c["tgt"]
        t32 = warp_time(c["u"] * (1 - R.T_EPS) + R.T_EPS, s=c["warp_s"])
        ref = R.prepare(s32, g32, c["u"], R.T_EPS, c["warp_s"], R.T_SCALE, c["pairing"], c["ids"], R.N_CLASSES, c["first_row"],
                        c["target_rows"], t_for_x=t32)
        g_rows = g32[ref["rows"]]
        worst["t"] = max(worst["t"], R.worst_ratio(t32, ref["t"], R.t_bound(c["u"], R.T_EPS, c["warp_s"])))
        x32 = (1 - t32).view(-1, 1) * s32 + t32.view(-1, 1) * g_rows
        worst["x"] = max(worst["x"], R.worst_ratio(x32, ref["x"], ref["x_bound"]))
        assert torch.equal(g_rows - s32, ref["v"].to(F32)), c["name"]          # one correctly rounded operation
        xi, vi, bi = R.interp(s32, g_rows, t32)
        assert torch.equal(xi, ref["x"]) and torch.equal(vi, ref["v"])
        worst["x (interp)"] = max(worst["x (interp)"], R.worst_ratio(x32, xi, bi))
    _report(worst)


def _mse_emulated(v, tgt, scale=None):
    """fp32, as mse_partial_kernel + mse_final[_acc]_kernel: (loss share, dv)."""
    n = v.numel()
    d = v.reshape(-1) - tgt.reshape(-1)
    total = R.partition_sum32(d * d)
    if scale is None:
        n32 = torch.tensor(float(n), dtype=F32)
        return total * (torch.tensor(1.0, dtype=F32) / n32), d * (torch.tensor(2.0, dtype=F32) / n32)
    return total * torch.tensor(scale / n, dtype=F32), d * torch.tensor(2.0 * scale / n, dtype=F32)


def test_loss_bounds_hold_for_torch_fp32_and_the_emulated_partition():
    info = {"loss (torch)": 0.0}
    worst = {"loss (partition)": 0.0, "dv (torch)": 0.0, "dv (partition)": 0.0, "micro loss": 0.0, "micro dv": 0.0}
    for name, v, tgt in R.loss_cases():
        ref_loss, ref_dv = R.mse(v, tgt)
        n = v.numel()
        vv = v.clone().requires_grad_(True)
        loss = torch.nn.MSELoss()(vv, tgt)
        loss.backward()
        emu_loss, emu_dv = _mse_emulated(v, tgt)
        bound = R.loss_rel_bound(n) * ref_loss
        info["loss (torch)"] = max(info["loss (torch)"], R.worst_ratio(loss.detach(), ref_loss, bound))
        worst["loss (partition)"] = max(worst["loss (partition)"], R.worst_ratio(emu_loss, ref_loss, bound))
        worst["dv (torch)"] = max(worst["dv (torch)"], R.worst_ratio(vv.grad, ref_dv, R.dv_bound(ref_dv)))
        worst["dv (partition)"] = max(worst["dv (partition)"], R.worst_ratio(emu_dv, ref_dv, R.dv_bound(ref_dv)))
    v, tgt = R.micro_case()
    whole_loss, whole_dv = R.mse(v, tgt)
    acc, acc_bound, lo, dvs = torch.zeros((), dtype=F32), 0.0, 0, []
    for rows in R.MICRO_ROWS:
        scale = float(torch.tensor(rows / sum(R.MICRO_ROWS), dtype=F32))        # the float the ABI carries
        share, dv = _mse_emulated(v[lo:lo + rows], tgt[lo:lo + rows], scale)
        ref_share = R.mse(v[lo:lo + rows], tgt[lo:lo + rows], rows / sum(R.MICRO_ROWS))[0]
        acc = acc + share
        acc_bound += float(R.loss_rel_bound(rows * R.MICRO_PER, extra=1) * ref_share) + R.U * float(acc)
        dvs.append(dv)
        lo += rows
    worst["micro loss"] = R.worst_ratio(acc, whole_loss, acc_bound)
    worst["micro dv"] = R.worst_ratio(torch.cat(dvs), whole_dv, R.dv_bound(whole_dv))
    _report(worst, info)


def _clip_emulated(g, g2, max_norm):
    parts = [g * g] + ([g2 * g2] if g2 is not None else [])
    norm = R.partition_sum32(*parts).sqrt()
    return norm, torch.minimum(torch.tensor(max_norm, dtype=F32) / (norm + torch.tensor(1e-6, dtype=F32)), torch.tensor(1.0, dtype=F32))


def test_clip_bounds_hold_for_torch_fp32_and_the_emulated_partition():
    worst = {"norm (partition)": 0.0, "coef (partition)": 0.0}
    info = {"norm (torch)": 0.0, "coef (torch)": 0.0}
    for name, g, g2, max_norm in R.clip_cases():
        norm, coef = R.clip(g, g2, max_norm)
        n, n2 = g.numel(), (0 if g2 is None else g2.numel())
        grads = {"a": g} if g2 is None else {"a": g, "b": g2}
        t_norm = R.to.grad_norm(grads)
        t_coef = R.to.clip_coef(t_norm, max_norm)
        e_norm, e_coef = _clip_emulated(g, g2, max_norm)
        for tag, got_norm, got_coef in (("torch", t_norm, t_coef), ("partition", e_norm, e_coef)):
            into = info if tag == "torch" else worst
            into[f"norm ({tag})"] = max(into[f"norm ({tag})"], R.worst_ratio(got_norm, norm, R.norm_rel_bound(n, n2) * norm))
            if float(coef) == 1.0:
                assert float(got_coef) == 1.0, (name, tag)
            else:
                into[f"coef ({tag})"] = max(into[f"coef ({tag})"], R.worst_ratio(got_coef, coef, R.coef_rel_bound(n, n2) * coef))
    _report(worst, info)


def test_adam_bounds_hold_for_torch_fp32():
    worst = {"p": 0.0, "exp_avg": 0.0, "exp_avg_sq": 0.0, "ema": 0.0, "ema (no gradient)": 0.0}
    for c in R.adam_cases():
        p, g, m, v, ema = R.adam_inputs(c["n"], c["state"], c["gscale"], c["seed"])
        assert float((g.square() * (1 - R.B2)).min()) > 1e-30
        hp = (c["coef"], c["lr"], R.B1, R.B2, R.EPS, c["step"], R.DECAY)
        ref = R.adam_ema(p, g, m, v, ema, *hp)
        got = R.adam_ema(p, g, m, v, ema, *hp, dtype=F32)
        bounds = R.adam_bounds(g, m, ema, c["coef"], c["lr"], R.B1, R.B2, R.EPS, c["step"], ref)
        for k, a, b, bd in zip(("p", "exp_avg", "exp_avg_sq", "ema"), got, ref, bounds):
            worst[k] = max(worst[k], R.worst_ratio(a, b, bd))
    p, g, m, v, ema = R.adam_inputs(4099, "nonzero", 1.0, 4999)
    hp = (1.0, 1e-4, R.B1, R.B2, R.EPS, 7, R.DECAY)
    ref = R.adam_ema(p, g, m, v, ema, *hp, apply_adam=False)
    got = R.adam_ema(p, g, m, v, ema, *hp, apply_adam=False, dtype=F32)
    worst["ema (no gradient)"] = R.worst_ratio(got[3], ref[3], R.adam_bounds(g, m, ema, 1.0, 1e-4, R.B1, R.B2, R.EPS, 7, ref, apply_adam=False)[3])
    _report(worst)


def test_a_float_one_minus_beta2_misses_the_exp_avg_sq_bound():
    """The gate has teeth: exp_avg_sq formed with 1.0f - 0.999f (1.3e-5 below (float)(1.0 - 0.999)) lies far outside the bound."""
    p, g, m, v, ema = R.adam_inputs(4099, "zero", 1.0, 4998)
    ref = R.adam_ema(p, g, m, v, ema, 1.0, 1e-4, R.B1, R.B2, R.EPS, 1, R.DECAY)
    one_minus_b2 = torch.tensor(1.0, dtype=F32) - torch.tensor(R.B2, dtype=F32)
    biased = v * torch.tensor(R.B2, dtype=F32) + one_minus_b2 * g * g
    bv = R.adam_bounds(g, m, ema, 1.0, 1e-4, R.B1, R.B2, R.EPS, 1, ref)[2]
    assert R.worst_ratio(biased, ref[2], bv) > 20


def test_horizon_inputs_cross_the_clip_threshold_both_ways():
    p0, grads = R.horizon_inputs()
    ref, norms = R.horizon_oracle(p0, grads, F64)
    got, _ = R.horizon_oracle(p0, grads, F32)
    active = sum(nm > R.HORIZON_MAX_NORM for nm in norms)
    assert 20 < active < R.HORIZON_STEPS - 20, active
    assert float(grads.abs().min()) >= 1e-13 and math.isfinite(float(grads.abs().max()))
    dv, dm, dp, de = R.horizon_figures(got, ref)
    print(f"{R.HORIZON_STEPS} steps, clip active on {active}: fp32 oracle vs fp64: exp_avg_sq rel {dv:.3e}, exp_avg abs {dm:.3e}, "
          f"p abs {dp:.3e}, ema abs {de:.3e}")
    assert dv < 1e-5
