"""flocoder_amd.sampling.log_likelihood(method="rk45") / invert_latents(method="rk45") on the CPU: the host path for any callable
(scipy's solve_ivp on the concatenated vector [x, a], torch.autograd.grad per evaluation), which is the literature's code shape and
documents what fc_unet_log_likelihood_rk45 implements, and the restatement the GPU golden comes from (tests/likelihood_rk45_ref.py).

Measured here (fp64, the Gaussian-to-Gaussian flow below, sigma = 2.5, D = 64, B = 4):
  |logp(1e-5) - exact| 2.2025e-3 and |logp(1e-5) - logp(1e-9)| 2.2026e-3 in every sample and both modes (nfev 20 against 74): 1.00 of the
  allowed factor 4; RK4 on 5 grid points 6.96e-3.
"""
import math

import numpy as np
import pytest
import torch

import likelihood_ref as lr
import likelihood_rk45_ref as rr
from conftest import load_golden
from flocoder_amd import sampling as S
from oracle.synth import synth_input

SIGMA, SHAPE, D = 2.5, (4, 4, 4, 4), 64


def _gauss_model(xx, time, cond=None):
    """v(x, t) = x (sigma - 1) / (1 + (sigma - 1) t): N(0, I) at t = 0 to N(0, sigma^2 I) at t = 1; diagonal Jacobian."""
    t = (time / 999).view(-1, 1, 1, 1)
    return xx * (SIGMA - 1) / (1 + (SIGMA - 1) * t)


def _gauss_case():
    x = SIGMA * synth_input("ll.gauss", SHAPE, 2).double()
    exact = -0.5 * x.flatten(1).pow(2).sum(1) / SIGMA ** 2 - 0.5 * D * math.log(2 * math.pi * SIGMA ** 2)
    return x, exact


def _gen():
    return torch.Generator().manual_seed(7)


def test_gaussian_flow_log_density_within_the_measured_solver_error_and_better_than_five_point_rk4():
    """The Jacobian is diagonal, so the Rademacher estimate is exact and the error is the solver's alone.  Its size is measured, not
    assumed: the same solve at 1e-9 stands in for the truth, |logp(1e-5) - exact| <= 4 max(|logp(1e-5) - logp(1e-9)|, 1e-9 |logp|) (the
    factor covers the tight solve's own error and sign).  And the control does something: strictly better than RK4 on 5 grid points."""
    x, exact = _gauss_case()
    for per_sample in (True, False):
        l5, z5, nfe5 = S.log_likelihood(_gauss_model, x, probe="rademacher", generator=_gen(), method="rk45", per_sample=per_sample)
        l9, _, nfe9 = S.log_likelihood(_gauss_model, x, probe="rademacher", generator=_gen(), method="rk45", rtol=1e-9, atol=1e-9,
                                       per_sample=per_sample)
        assert l5.dtype == torch.float64 and z5.dtype == torch.float64 and z5.shape == x.shape and nfe9 > nfe5 >= 8 and (nfe5 - 2) % 6 == 0
        err, gap = (l5 - exact).abs(), (l5 - l9).abs()
        print(f"per_sample={per_sample}: nfe {nfe5} / {nfe9}; |logp(1e-5) - exact| {err.tolist()}, |logp(1e-5) - logp(1e-9)| {gap.tolist()}")
        assert bool((err <= 4 * torch.maximum(gap, 1e-9 * l5.abs())).all()), (err, gap)
        # z is the N(0, I) preimage: x / sigma
        assert float((z5 - x / SIGMA).abs().max()) <= 1e-3
        l_rk4, _, _ = S.log_likelihood(_gauss_model, x, n_steps=5, generator=_gen())
        print(f"  RK4 on 5 points: {(l_rk4 - exact).abs().tolist()}")
        assert bool((err < (l_rk4 - exact).abs()).all())


def test_per_sample_on_a_batch_equals_separate_calls_exactly():
    x, _ = _gauss_case()
    x = x * torch.tensor([1.0, 0.05, 3.0, 0.6], dtype=torch.float64).view(-1, 1, 1, 1)     # samples that step differently
    eps = torch.where(synth_input("llrk45.cpu.eps", SHAPE, 1) >= 0, 1.0, -1.0).double()
    logp, z, nfe = S.log_likelihood(_gauss_model, x, probe=eps, method="rk45", per_sample=True)
    nfes = []
    for b in range(x.shape[0]):
        lb, zb, nb = S.log_likelihood(_gauss_model, x[b:b + 1], probe=eps[b:b + 1], method="rk45", per_sample=True)
        assert torch.equal(lb, logp[b:b + 1]) and torch.equal(zb, z[b:b + 1])
        nfes.append(nb)
    assert nfe == max(nfes) and len(set(nfes)) > 1
    # the coupled solve is another problem: one step size for the batch
    lc, _, nc = S.log_likelihood(_gauss_model, x, probe=eps, method="rk45", per_sample=False)
    assert not torch.equal(lc, logp) and float((lc - logp).abs().max()) < 1e-2
    # inversion: the same solve without the a-track is solve_ivp on x alone
    zi, ni = S.invert_latents(_gauss_model, x, method="rk45", per_sample=True)
    for b in range(x.shape[0]):
        zb, _ = S.invert_latents(_gauss_model, x[b:b + 1], method="rk45")
        assert torch.equal(zb, zi[b:b + 1])
    assert float((zi - x / SIGMA).abs().max()) <= 1e-3 and ni >= 8
    zc, _ = S.invert_latents(_gauss_model, x, method="rk45", per_sample=False)
    assert float((zc - zi).abs().max()) <= 1e-3


def test_refusals_and_the_untouched_rk4_default():
    x, _ = _gauss_case()
    with pytest.raises(ValueError, match="guidance"):
        S.log_likelihood(_gauss_model, x, method="rk45", cfg_strength=3.0)
    with pytest.raises(ValueError, match="atol"):
        S.log_likelihood(_gauss_model, x, method="rk45", atol=-1.0)
    with pytest.raises(ValueError, match="atol"):
        S.invert_latents(_gauss_model, x, method="rk45", atol=-1.0)
    with pytest.warns(UserWarning, match="rtol"):
        S.log_likelihood(_gauss_model, x, method="rk45", rtol=1e-16, atol=1e-3)
    with pytest.raises(ValueError, match="method"):
        S.log_likelihood(_gauss_model, x, method="dopri8")
    with pytest.raises(ValueError, match="method"):
        S.invert_latents(_gauss_model, x, method="euler")
    with pytest.raises(ValueError, match="t_end"):
        S.log_likelihood(_gauss_model, x, method="rk45", t_end=1.0)
    with pytest.raises(ValueError, match="shape"):
        S.log_likelihood(_gauss_model, x, method="rk45", probe=torch.ones(4, 4, 4, 5))
    from flocoder_amd.unet import Unet
    m = Unet(dim=8, channels=4, n_classes=0).eval()
    with pytest.raises(RuntimeError):
        S.log_likelihood(m, torch.zeros(1, 4, 8, 8), method="rk45")
    with pytest.raises(RuntimeError):
        S.invert_latents(m, torch.zeros(1, 4, 8, 8), method="rk45")
    # method="rk4" (the default) is today's loop, bit for bit
    eps = S._make_probe("rademacher", x, _gen())
    ref, zr, _, _ = S._log_likelihood_torch(_gauss_model, x, S._reverse_grid(7, x.dtype), None, eps)
    for kw in ({}, {"method": "rk4"}, {"method": "rk4", "rtol": 1e-3, "per_sample": False}):
        logp, z, nfe = S.log_likelihood(_gauss_model, x, n_steps=7, generator=_gen(), **kw)
        assert torch.equal(logp, ref) and torch.equal(z, zr) and nfe == 24
    # t_end: the solve stops there
    lt, zt, _ = S.log_likelihood(_gauss_model, x, method="rk45", t_end=0.5, generator=_gen())
    assert float((zt - x * (1 + (SIGMA - 1) * 0.5) / SIGMA).abs().max()) <= 1e-3 and torch.isfinite(lt).all()


@pytest.mark.timeout(600)
def test_the_restatements_counters_are_solve_ivps_on_the_concatenated_vector():
    """tests/likelihood_rk45_ref.py steps scipy's RK45 object by hand (to tell accepted evaluations apart); a plain solve_ivp call on
    [x, a] with a hand-written field must give its counters, z and a -- which pins n = m + spg in the norms and the a-component's scale
    atol + rtol max(|a|, |a_new|) as scipy's own -- and the public host path must agree with both."""
    from scipy.integrate import solve_ivp
    sd, x, eps, cond = rr.case_inputs("d8mask")
    sd64 = {k: v.double() for k, v in sd.items()}
    x, eps = x.double(), eps.double()
    tol, t_end = 1e-2, 0.5                                    # a short solve: the identity under test depends on neither
    for per_sample in (False, True):
        ref = rr.log_likelihood_rk45_ref(sd64, x, cond, eps, per_sample=per_sample, t1=t_end, rtol=tol, atol=tol)
        groups = [(slice(b, b + 1), rr.sample_cond(cond, b)) for b in range(x.shape[0])] if per_sample else [(slice(0, x.shape[0]), cond)]
        for gi, (rows, cg) in enumerate(groups):
            xg, eg = x[rows], eps[rows]
            n = xg.numel()

            def f(t, y):
                v, _, d = lr.stage_eval(sd64, torch.from_numpy(y[:n].reshape(xg.shape).copy()), t, cg, eg)
                return np.concatenate([v.numpy().reshape(-1), d.numpy()])

            sol = solve_ivp(f, (1.0, t_end), np.concatenate([xg.numpy().reshape(-1), np.zeros(xg.shape[0])]), method="RK45", rtol=tol, atol=tol)
            acc = len(sol.t) - 1
            assert sol.success and ref.counts[gi].tolist() == [sol.nfev, acc, (sol.nfev - 2) // 6 - acc]
            assert np.array_equal(sol.y[n:, -1], ref.a[rows].numpy()) and np.array_equal(sol.y[:n, -1], ref.z[rows].numpy().reshape(-1))
        assert bool((ref.gsum > 0).all()) and ref.counts.shape == (len(groups), 3)
        logp, z, nfe = S.log_likelihood(lr.oracle_model(sd64), x, cond=cond, probe=eps, method="rk45", rtol=tol, atol=tol, per_sample=per_sample,
                                      t_end=t_end)
        assert torch.equal(logp, ref.logp) and torch.equal(z, ref.z) and nfe == int(ref.counts[:, 0].max())


def test_the_golden_holds_what_the_gpu_test_needs():
    g = load_golden("ll_rk45_scipy_oracle")
    assert float(g["tol"]) == rr.RTOL and float(g["tight_tol"]) < rr.RTOL
    rejected = 0
    for cid, (_, _, _, bsz, hw, _, _) in rr.CASES.items():
        for mode, groups in (("coupled", 1), ("ps", bsz)):
            assert g[f"{cid}.{mode}.counts"].shape == (groups, 3) and g[f"{cid}.{mode}.z"].shape == (bsz, 4, hw, hw)
            for k in ("a", "logp", "gsum"):
                assert g[f"{cid}.{mode}.{k}"].shape == (bsz,) and np.isfinite(g[f"{cid}.{mode}.{k}"]).all()
            assert (g[f"{cid}.{mode}.counts"][:, 2] >= 1).all()               # every solve exercises the rejection path
            # the case was admitted by the reference's own sensitivity to fp32 evaluation (likelihood_rk45_ref.FP32_AGREEMENT)
            assert g[f"{cid}.{mode}.z32_rel"].shape == (bsz,) and (g[f"{cid}.{mode}.z32_rel"] <= rr.FP32_AGREEMENT).all()
            assert np.array_equal(g[f"{cid}.{mode}.counts32"], g[f"{cid}.{mode}.counts"])
            rejected += int(g[f"{cid}.{mode}.counts"][:, 2].sum())
        assert g[f"{cid}.a_tight"].shape == (bsz,)
    assert rejected >= 1
