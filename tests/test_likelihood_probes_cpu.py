"""K Hutchinson probes in one likelihood solve on the CPU: the generic-model (torch / scipy) paths of sampling.log_likelihood, the NumPy
probe field (flocoder_amd.noise.probe_field) and the golden of the GPU test (tools/make_ll_probes_golden.py).

Bounds: closed forms where there is one (the diagonal Gaussian flow of tests/test_likelihood_cpu.py with its tolerances; a dense linear
field whose divergence integral is -tr(A) exactly); equalities of bits against the single-probe code; and for the per-probe by-products
of the adaptive solve |mean_k a_k - a| <= 1e-11 (1 + max_k |a_k|): both sides are the same linear functional of the d_{s,k}, apart by the
fp64 rounding of about ten operations per step over at most a few hundred steps."""
import math

import numpy as np
import pytest
import torch

import likelihood_probes_ref as pr
import likelihood_rk45_ref as rr
from conftest import load_golden
from flocoder_amd import noise as N
from flocoder_amd import sampling as S
from flocoder_amd.metrics import bits_per_dim_stderr
from oracle.synth import synth_input

SIGMA, SHAPE, D = 2.5, (4, 4, 4, 4), 64


def _gauss_model(xx, time, cond=None):
    t = (time / 999).view(-1, 1, 1, 1)
    return xx * (SIGMA - 1) / (1 + (SIGMA - 1) * t)


def _gauss_case():
    x = SIGMA * synth_input("ll.gauss", SHAPE, 2).double()
    return x, -0.5 * x.flatten(1).pow(2).sum(1) / SIGMA ** 2 - 0.5 * D * math.log(2 * math.pi * SIGMA ** 2)


def _gen(seed=7):
    return torch.Generator().manual_seed(seed)


def _linear_case():
    """v = A x on D = 16 unknowns (fp64, dense A): dv/dx = A everywhere, so d = eps^T A eps at every evaluation and the divergence
    integral from 1 to 0 is -tr(A) exactly."""
    A = 0.3 * torch.randn(16, 16, generator=_gen(21), dtype=torch.float64)
    model = lambda x, time, cond=None: (x.flatten(1) @ A.T).view_as(x)
    return A, model, synth_input("llp.lin", (2, 4, 2, 2), 4).double()


def test_gaussian_flow_four_probes_have_no_spread_and_the_exact_log_density():
    """Diagonal Jacobian: every Rademacher probe gives the divergence exactly, so the standard error is rounding and logp keeps the
    tolerances of the single-probe tests (tests/test_likelihood_cpu.py at 33 points; tests/test_likelihood_rk45_cpu.py's measured solver
    error) on both host paths."""
    x, exact = _gauss_case()
    logp, z, nfe, info = S.log_likelihood(_gauss_model, x, n_steps=33, n_probes=4, generator=_gen(), return_info=True)
    assert nfe == 4 * 32 and info["n_probes"] == 4 and info["a_probes"].shape == (4, 4)
    assert float(info["logp_stderr"].max()) <= 1e-9
    assert float((logp - exact).abs().max()) <= 1e-5 * float(exact.abs().min())
    for per_sample in (True, False):
        l5, _, nfe5, i5 = S.log_likelihood(_gauss_model, x, n_probes=4, generator=_gen(), method="rk45", per_sample=per_sample, return_info=True)
        l9, _, _ = S.log_likelihood(_gauss_model, x, n_probes=4, generator=_gen(), method="rk45", rtol=1e-9, atol=1e-9, per_sample=per_sample)
        l1, _, nfe1 = S.log_likelihood(_gauss_model, x, generator=_gen(), method="rk45", per_sample=per_sample)
        assert float(i5["logp_stderr"].max()) <= 1e-9 and nfe5 == nfe1                  # nfe counts velocity evaluations: not K times more
        err, gap = (l5 - exact).abs(), (l5 - l9).abs()
        assert bool((err <= 4 * torch.maximum(gap, 1e-9 * l5.abs())).all()), (err, gap)
    assert torch.equal(bits_per_dim_stderr(info["logp_stderr"], D), info["logp_stderr"] / (D * math.log(2.0)))


def test_rk4_mean_of_k_probes_is_the_mean_of_k_calls_and_brackets_the_trace():
    A, model, x = _linear_case()
    probes = torch.where(torch.randn(3, *x.shape, generator=_gen(3), dtype=torch.float64) >= 0, 1.0, -1.0)
    logp, z, nfe, info = S.log_likelihood(model, x, n_steps=6, probe=probes, return_info=True)
    singles = [S.log_likelihood(model, x, n_steps=6, probe=probes[k], return_info=True) for k in range(3)]
    for k in range(3):
        assert torch.equal(info["a_probes"][k], singles[k][3]["a"]) and torch.equal(z, singles[k][1])
    mean = sum(s[3]["a"] for s in singles) / 3
    assert float((info["a"] - mean).abs().max()) <= 1e-12 and float((logp - sum(s[0] for s in singles) / 3).abs().max()) <= 1e-12 * float(logp.abs().max())
    assert bool(torch.isnan(singles[0][3]["logp_stderr"]).all()) and singles[0][3]["n_probes"] == 1
    k1 = S.log_likelihood(model, x, n_steps=6, probe=probes[:1], return_info=True)
    assert torch.equal(k1[0], singles[0][0]) and bool(torch.isnan(k1[3]["logp_stderr"]).all())
    # the estimator against the exact integral -tr(A), K = 64 drawn probes of a fixed seed; every a_k is -eps_k^T A eps_k
    for kind in ("rademacher", "gaussian"):
        _, _, _, i64 = S.log_likelihood(model, x, n_steps=6, n_probes=64, probe=kind, generator=_gen(5), return_info=True)
        dev = (i64["a"] + torch.trace(A)).abs()
        assert bool((dev <= 5 * i64["logp_stderr"]).all()), (kind, dev.tolist(), i64["logp_stderr"].tolist())
        assert bool((i64["logp_stderr"] > 0).all())
    # the drawn probes: the first of K is the draw a K = 1 call makes
    _, _, _, i1 = S.log_likelihood(model, x, n_steps=6, generator=_gen(5), return_info=True)
    _, _, _, i2 = S.log_likelihood(model, x, n_steps=6, n_probes=2, generator=_gen(5), return_info=True)
    assert torch.equal(i2["a_probes"][0], i1["a"])


def _parent_rk45_host(model, latents, cond, eps, rtol, atol, per_sample, t_end=0.0, t_scale=999):
    """The single-probe host path as it stood before several probes: scipy's solve_ivp on [x, a] -> (z, a, nfe)."""
    from scipy import integrate
    z, a = latents.detach().clone(), torch.zeros(latents.shape[0], dtype=torch.float64)
    nfevs = []
    for rows, cond_g in S._host_rk45_groups(latents, cond, per_sample):
        xg, eg = latents[rows].detach(), eps[rows]
        shape, n, e64 = tuple(xg.shape), xg.numel(), eps[rows].double()

        def ode_func(t, y):
            with torch.enable_grad():
                xr = torch.from_numpy(np.ascontiguousarray(y[:n]).reshape(shape)).to(dtype=xg.dtype).requires_grad_(True)
                v = model(xr, torch.full((shape[0],), float(t), dtype=xg.dtype) * t_scale, cond=cond_g)
                g, = torch.autograd.grad(v, xr, eg)
            return np.concatenate([v.detach().double().numpy().reshape(-1), (e64 * g.double()).flatten(1).sum(dim=1).numpy()])

        y0 = np.concatenate([xg.double().numpy().reshape(-1), np.zeros(shape[0])])
        sol = integrate.solve_ivp(ode_func, (1.0, t_end), y0, rtol=rtol, atol=atol, method="RK45")
        assert sol.success
        z[rows] = torch.from_numpy(sol.y[:n, -1].reshape(shape).copy()).to(dtype=xg.dtype)
        a[rows] = torch.from_numpy(sol.y[n:, -1].copy())
        nfevs.append(int(sol.nfev))
    return z, a, max(nfevs)


def _nonlinear_model(x, time, cond=None):
    """any callable: a field with a dense, state-dependent Jacobian"""
    t = (time / 999).view(-1, 1, 1, 1)
    return torch.tanh(x.roll(1, 1) * 0.8 + x.roll(1, 3) * 0.5) * (1.5 - t) + 0.3 * x.flip(2)


@pytest.mark.parametrize("per_sample", [True, False])
def test_host_rk45_one_probe_identical_probes_and_by_products(per_sample):
    x = synth_input("llp.nl", (3, 4, 4, 4), 6).double()
    probes = torch.where(torch.randn(3, *x.shape, generator=_gen(9), dtype=torch.float64) >= 0, 1.0, -1.0)
    zp, ap, nfep = _parent_rk45_host(_nonlinear_model, x, None, probes[0], 1e-5, 1e-5, per_sample)
    # K = 1: the bits of the function as it stood
    logp, z, a, nfe, _ = S._log_likelihood_rk45_host(_nonlinear_model, x, None, probes[0], 1e-5, 1e-5, per_sample)
    assert torch.equal(z, zp) and torch.equal(a, ap) and nfe == nfep
    lp_pub, z_pub, nfe_pub = S.log_likelihood(_nonlinear_model, x, probe=probes[0], method="rk45", per_sample=per_sample)
    assert torch.equal(lp_pub, logp) and torch.equal(z_pub, zp) and nfe_pub == nfep
    # K copies of one probe: the single-probe result and counters (sums of 2 or 4 equal doubles and the division are exact)
    for k in (2, 4):
        lk, zk, ak, nk, apk = S._log_likelihood_rk45_host(_nonlinear_model, x, None, probes[:1].expand(k, *x.shape), 1e-5, 1e-5, per_sample)
        assert torch.equal(zk, zp) and torch.equal(ak, ap) and nk == nfep and torch.equal(lk, logp)
        assert float((apk - ak).abs().max()) <= 1e-11 * (1 + float(apk.abs().max()))
    # distinct probes: the by-products average to the state's a
    l3, z3, nfe3, info = S.log_likelihood(_nonlinear_model, x, probe=probes, method="rk45", per_sample=per_sample, return_info=True)
    a_probes, a3 = info["a_probes"], info["a"]
    assert a_probes.shape == (3, 3) and not torch.equal(a_probes[0], a_probes[1])
    assert bool(((a_probes.mean(0) - a3).abs() <= 1e-11 * (1 + a_probes.abs().max(0).values)).all())
    ref_se = torch.sqrt(((a_probes - a3) ** 2).sum(0) / 6)
    assert torch.allclose(info["logp_stderr"], ref_se, rtol=1e-14, atol=0) and bool((ref_se > 0).all())


def test_numpy_probe_field():
    ids = np.array([7, 0, 2 ** 33 + 1, -3], dtype=np.int64)
    for kind in ("rademacher", "gaussian"):
        f = N.probe_field(3, 5, ids, 256, kind)
        assert f.shape == (4, 256) and f.dtype == np.float32
        assert np.array_equal(N.probe_field(3, 5, ids, 256, kind), f)                                # deterministic
        perm = np.array([2, 0, 3, 1])
        assert np.array_equal(N.probe_field(3, 5, ids[perm], 256, kind), f[perm])                    # permuting sample_ids permutes rows
        assert np.array_equal(N.probe_field(3, 5, [7], 256, kind)[0], f[0])                          # not the batch
        assert np.array_equal(N.probe_field(3, 5, ids, 512, kind)[:, :256], f)                       # the position, not the sample's size
        for other in (N.probe_field(4, 5, ids, 256, kind), N.probe_field(3, 6, ids, 256, kind), N.probe_field(3 + 2 ** 32, 5, ids, 256, kind)):
            assert not np.array_equal(other, f)
        assert np.array_equal(N.probe_field(3, 5, ids, 256, N.PROBE_KINDS[kind]), f)
    r = N.probe_field(3, 0, ids, 4096)
    assert np.isin(r, (-1.0, 1.0)).all() and abs(r.mean()) <= 5 / math.sqrt(r.size)
    # a likelihood seed does not replay the SDE sampler's normals of the same seed
    z, gsn = N.normal_field(3, 5, ids, 4096), N.probe_field(3, 5, ids, 4096, "gaussian")
    assert not np.array_equal(gsn, z.astype(np.float32)) and abs(np.corrcoef(gsn.ravel(), z.ravel())[0, 1]) < 5 / math.sqrt(z.size)
    assert abs(np.corrcoef(r.ravel(), np.sign(N.normal_field(3, 0, ids, 4096)).ravel())[0, 1]) < 5 / math.sqrt(r.size)
    assert np.array_equal(gsn, N.normal_field((3 + N.PROBE_KEY_OFFSET) % 2 ** 64, 5, ids, 4096).astype(np.float32))
    with pytest.raises(ValueError):
        N.probe_field(0, 0, [0], 6)
    with pytest.raises(ValueError):
        N.probe_field(0, 0, [0], 8, "sobol")
    # the torch wrapper on the CPU, and the public function fed by it: a sample's probes follow its id
    t = S.probe_field(3, 5, torch.from_numpy(ids), (4, 4, 8, 8))
    assert torch.equal(t.flatten(1), torch.from_numpy(N.probe_field(3, 5, ids, 256)))
    A, model, x = _linear_case()
    l2, _, _, i2 = S.log_likelihood(model, x, n_steps=4, n_probes=2, probe_seed=3, sample_ids=[9, 5], return_info=True)
    l1, _, _, i1 = S.log_likelihood(model, x[1:], n_steps=4, n_probes=2, probe_seed=3, sample_ids=[5], return_info=True)
    assert torch.equal(i2["a_probes"][:, 1:], i1["a_probes"]) and torch.equal(i2["logp_stderr"][1:], i1["logp_stderr"])


def test_argument_errors():
    A, model, x = _linear_case()
    probes = torch.ones(3, *x.shape, dtype=torch.float64)
    with pytest.raises(ValueError, match="n_probes"):
        S.log_likelihood(model, x, n_steps=3, probe=probes, n_probes=2)
    with pytest.raises(ValueError, match="generator"):
        S.log_likelihood(model, x, n_steps=3, probe_seed=1, generator=_gen())
    for k in (0, 65):
        with pytest.raises(ValueError, match="64"):
            S.log_likelihood(model, x, n_steps=3, n_probes=k)
    with pytest.raises(ValueError, match="probe_seed"):
        S.log_likelihood(model, x, n_steps=3, sample_ids=[0, 1])
    with pytest.raises(ValueError, match="sample_ids"):
        S.log_likelihood(model, x, n_steps=3, probe_seed=1, sample_ids=[0, 1, 2])
    assert len(S.log_likelihood(model, x, n_steps=3, probe=probes, n_probes=3)) == 3


def test_the_golden_holds_what_the_gpu_test_needs():
    g = load_golden("ll_probes_rk45_scipy_oracle")
    assert float(g["tol"]) == rr.RTOL and float(g["tight_tol"]) < rr.RTOL
    for cid, (_, _, _, bsz, hw, _, _) in rr.CASES.items():
        assert tuple(g[f"{cid}.probe_seeds"]) == tuple(pr.PROBE_SEEDS[cid])
        _, x, eps, _ = pr.case_inputs(cid)
        assert eps.shape == (pr.N_PROBES, bsz, 4, hw, hw) and torch.equal(eps[0], rr.case_inputs(cid)[2])       # the first probe is the single-probe golden's
        for mode, groups in (("coupled", 1), ("ps", bsz)):
            assert g[f"{cid}.{mode}.counts"].shape == (groups, 3) and g[f"{cid}.{mode}.z"].shape == (bsz, 4, hw, hw)
            for k in ("a", "logp"):
                assert g[f"{cid}.{mode}.{k}"].shape == (bsz,) and np.isfinite(g[f"{cid}.{mode}.{k}"]).all()
            for k in ("gsum", "a_probes"):
                assert g[f"{cid}.{mode}.{k}"].shape == (pr.N_PROBES, bsz) and np.isfinite(g[f"{cid}.{mode}.{k}"]).all()
            # admission (likelihood_rk45_ref.FP32_AGREEMENT): fp32 against fp64 oracle, equal counters, rejected steps in every solve
            assert (g[f"{cid}.{mode}.counts"][:, 2] >= 1).all()
            assert g[f"{cid}.{mode}.z32_rel"].shape == (bsz,) and (g[f"{cid}.{mode}.z32_rel"] <= rr.FP32_AGREEMENT).all()
            assert np.array_equal(g[f"{cid}.{mode}.counts32"], g[f"{cid}.{mode}.counts"])
            ap, a = g[f"{cid}.{mode}.a_probes"], g[f"{cid}.{mode}.a"]
            assert (np.abs(ap.mean(0) - a) <= 1e-11 * (1 + np.abs(ap).max(0))).all()
        assert g[f"{cid}.a_tight"].shape == (bsz,)
