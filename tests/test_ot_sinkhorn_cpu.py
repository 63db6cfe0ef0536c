"""The entropic OT plan's reference (tests/ot_sinkhorn_ref.py) on the CPU: the log-domain restatement against kernel-form
Sinkhorn-Knopp where that form does not underflow, the plan's identities and cost bounds, the margin that makes the device's stopping
iteration unambiguous, the sampler (two forms, chi-square), the host uniforms and the host logic of ``flocoder_amd.ot``."""
import numpy as np
import pytest
import torch

import ot_sinkhorn_ref as R

ALL = R.CASES + R.STUCK_CASES


@pytest.mark.parametrize("case", R.CASES)
def test_log_domain_equals_kernel_form_where_that_does_not_underflow(case):
    B, D, reg, normalised, _ = case
    c = R.host_cost(B, D, normalised).astype(np.float64)
    if reg != 0.05:                                       # max(C) / reg <= 20 is where exp(-C / reg) >= 2e-9 keeps its digits
        reg = 0.05
        _, f, g, it, _, _ = R.sinkhorn(c, reg, 1000, R.STOP_THR)
    else:
        _, f, g, it, _, _, _ = R.host_solution(case)
    assert c.max() / reg <= 20.0 + 1e-12
    fk, gk = R.sinkhorn_knopp(c, reg, it)
    shift = float(np.mean(f - fk))                        # (f + s, g - s) is the same plan
    print(f"{case}: {it} iterations, |f - fk| {np.abs(f - fk - shift).max():.2e}, |g - gk| {np.abs(g - gk + shift).max():.2e}")
    assert np.abs(f - fk - shift).max() <= 1e-10 * reg
    assert np.abs(g - gk + shift).max() <= 1e-10 * reg


@pytest.mark.parametrize("case", ALL)
def test_plan_identities_and_cost_bounds(case):
    B, D, reg, normalised, max_iter = case
    c = R.host_cost(B, D, normalised).astype(np.float64)
    plan, f, g, it, conv, err, trace = R.host_solution(case)
    assert it == (trace[-1][0] if trace else 0) and it % 10 == 0 and it <= R.round_iters(max_iter)
    assert conv == (err < R.STOP_THR) and (conv or it == R.round_iters(max_iter))
    assert np.allclose(plan, np.exp((f[:, None] + g[None, :] - c) / reg), rtol=0, atol=0)
    assert np.abs(plan.sum(1) - 1.0 / B).max() <= 1e-12          # the row half came last
    assert R.col_err(c, f, g, reg) == err
    lo, hi = R.cost_bounds(c)
    pc = float((plan * c).sum())
    slack = np.sqrt(B) * err * c.max()
    print(f"{case}: {it} iterations, err {err:.3e}, <P, C> = {pc:.6f} in [{lo:.6f}, {hi:.6f}]")
    assert lo - slack <= pc <= hi + slack


@pytest.mark.parametrize("case", ALL)
def test_no_check_lands_within_one_percent_of_the_threshold(case):
    """So that the device, whose potentials differ from the restatement's in the last bits, cannot stop a block earlier or later."""
    trace = R.host_solution(case)[6]
    assert trace and all(abs(err - R.STOP_THR) > 0.01 * R.STOP_THR for _, err in trace), trace


def test_expected_iteration_counts():
    its = {c: R.host_solution(c)[3] for c in ALL}
    assert all(10 <= its[c] <= 120 for c in R.CASES if c[2] == 0.05), its
    assert its[(128, 32, 0.01, True, 1000)] > 200
    for c in R.STUCK_CASES:
        assert its[c] == 1000 and not R.host_solution(c)[4]


def test_max_iter_is_rounded_up_to_the_check_period():
    c = R.host_cost(7, 16, True)
    assert R.sinkhorn(c, 0.05, 1, 0.0)[3] == 10 and R.sinkhorn(c, 0.05, 11, 0.0)[3] == 20 and R.sinkhorn(c, 0.05, 20, 0.0)[3] == 20


def test_sentinels_and_equal_costs():
    plan, f, g, it, conv, err = R.sinkhorn(R.equal_matrix(70), 0.05)
    assert conv and it == 10 and np.abs(plan - 1.0 / 4900).max() < 1e-15
    assert np.array_equal(R.plan_pairing(plan.astype(np.float32)), np.arange(70))      # all equal: ties go to the lowest column
    n = R.normalise(np.array([[1.0, np.inf], [4.0, 2.0]], dtype=np.float32))
    assert n[0, 1] == np.float32(R.X.FLT_MAX) and n[1, 0] == 1.0 and n[0, 0] == 0.25
    assert np.array_equal(R.normalise(np.zeros((3, 3), np.float32)), np.zeros((3, 3), np.float32))


# ---- sampler --------------------------------------------------------------------------------------------------------------------
def _plan32(B, D, reg):
    return R.sinkhorn(R.host_cost(B, D, True), reg)[0].astype(np.float32)


@pytest.mark.parametrize("B,D,reg", R.SAMPLE_CASES)
def test_two_level_search_equals_the_flat_cdf(B, D, reg):
    from flocoder_amd.noise import plan_uniforms
    p = _plan32(B, D, reg)
    for seed, draw, n in ((12345, 0, 4096), (12345, 7, B), (2 ** 63 + 5, 2 ** 32 - 1, 1)):
        u = plan_uniforms(seed, draw, n)
        i, j, ok = R.sample_two_level(p, u)
        fi, fj = R.sample_flat(p, u)
        assert ok and np.array_equal(i, fi) and np.array_equal(j, fj)
        assert i.min() >= 0 and i.max() < B and j.min() >= 0 and j.max() < B


def test_sampler_edges():
    p = np.array([[0.0, 0.5], [0.5, 0.0]], dtype=np.float32)
    u = np.array([2.0 ** -54, 0.25, 0.5 - 2.0 ** -54, 0.5, 0.75, 1.0])
    i, j, ok = R.sample_two_level(p, u)
    assert ok and i.tolist() == [0, 0, 0, 1, 1, 1] and j.tolist() == [1, 1, 1, 0, 0, 1]        # u = 1: clamped to the last cell
    for bad in (np.zeros((3, 3), np.float32), np.full((3, 3), np.nan, np.float32), np.full((3, 3), np.inf, np.float32)):
        i, j, ok = R.sample_two_level(bad, np.full(5, 0.5))
        assert not ok and i.tolist() == [0, 1, 2, 0, 1] and j.tolist() == [0, 1, 2, 0, 1]


def test_sampler_chi_square():
    """65536 draws from the B = 8 plan; cells with expectation under 5 are pooled into one."""
    from scipy.stats import chi2
    from flocoder_amd.noise import plan_uniforms
    p = _plan32(8, 16, 0.05)
    n = 65536
    i, j, _ = R.sample_two_level(p, plan_uniforms(12345, 0, n))
    obs = np.bincount(i * 8 + j, minlength=64).astype(np.float64)
    exp = p.astype(np.float64).ravel() / p.astype(np.float64).sum() * n
    small = exp < 5
    o = np.append(obs[~small], obs[small].sum())
    e = np.append(exp[~small], exp[small].sum())
    if e[-1] == 0:
        o, e = o[:-1], e[:-1]
    stat = float(((o - e) ** 2 / e).sum())
    bound = float(chi2.ppf(1 - 1e-6, len(e) - 1))
    print(f"chi-square {stat:.1f} against {bound:.1f} at {len(e) - 1} dof (min expectation {exp.min():.2f}, {int(small.sum())} cells pooled)")
    assert stat < bound


def test_uniforms53_bit_recipe_and_range():
    from flocoder_amd import noise as N
    w = N.philox4x32(np.array([[k, 3, N.PLAN_TAG, 0xFFFFFFFF] for k in range(5)], dtype=np.uint64), np.array([0x9abcdef0, 0x12345678], dtype=np.uint64))
    u = N.plan_uniforms(0x123456789abcdef0, 3, 5)
    for k in range(5):
        want = ((int(w[k, 0]) >> 5) * 2 ** 26 + (int(w[k, 1]) >> 6) + 0.5) / 2 ** 53
        assert u[k] == want
    assert N.uniforms53(0, 0) == 2.0 ** -54 and N.uniforms53(0xFFFFFFFF, 0xFFFFFFBF) < 1.0
    assert N.uniforms53(0xFFFFFFFF, 0xFFFFFFFF) == 1.0          # the one pair of words whose sum rounds up: the inversion's clamp takes it
    big = N.plan_uniforms(7, 0, 65536)
    assert big.min() > 0.0 and big.max() < 1.0 and abs(big.mean() - 0.5) < 0.01
    assert not np.array_equal(N.plan_uniforms(7, 1, 16), big[:16]) and not np.array_equal(N.plan_uniforms(8, 0, 16), big[:16])
    assert np.array_equal(N.plan_uniforms(7, 0, 16), big[:16])                        # a value depends on (seed, draw, k) alone
    # the region is disjoint from the SDE field's: there counter word 3 is a sample id's high word, all ones only for negative ids
    assert N.field_words(7, 0, [-1], 4)[0, 0].tolist() != N.philox4x32(np.array([0, 0, N.PLAN_TAG, 0xFFFFFFFF], np.uint64), np.array([7, 0], np.uint64)).tolist()
    with pytest.raises(ValueError):
        N.plan_uniforms(0, -1, 4)
    with pytest.raises(ValueError):
        N.plan_uniforms(0, 2 ** 32, 4)


def test_plan_pairing_sweep():
    p = np.array([[0.1, 0.3, 0.3], [0.0, 0.9, 0.2], [0.5, 0.5, 0.5]], dtype=np.float32)
    assert R.plan_pairing(p).tolist() == [1, 2, 0]
    perm = R.plan_pairing(_plan32(64, 32, 0.05))
    assert R.X.is_permutation(perm, 64)


# ---- host logic of flocoder_amd.ot ----------------------------------------------------------------------------------------------
def test_host_logic_raises_before_the_device_is_touched():
    from flocoder_amd import OTPlanSampler, compute_ot_pairing, compute_ot_plan, sample_plan
    from flocoder_amd.train import batch_to_data
    x = torch.zeros(4, 3)
    from flocoder_amd.ot import compute_ot_pairing_sinkhorn
    for call in (lambda: compute_ot_plan(x, x), lambda: sample_plan(torch.zeros(4, 4)), lambda: compute_ot_pairing_sinkhorn(x, x),
                 lambda: OTPlanSampler("sinkhorn").sample_plan(x, x), lambda: OTPlanSampler("exact").get_map(x, x)):
        with pytest.raises(RuntimeError, match="no CPU path"):                       # CPU tensors raise, as everywhere else
            call()
    with pytest.raises(ValueError, match="no CPU path"):                             # through the dispatcher: the error type it had for this method
        compute_ot_pairing(x, x, method="sinkhorn")
    # argument errors come before the device check, so they show here too
    for bad in (dict(reg=0.0), dict(reg=-1.0), dict(reg=float("nan")), dict(max_iter=0), dict(max_iter=10001), dict(stop_thr=-1.0)):
        with pytest.raises(ValueError):
            compute_ot_plan(x, x, **bad)
    for a, b in ((torch.zeros(4, 3), torch.zeros(5, 3)), (torch.zeros(0, 3), torch.zeros(0, 3)), (torch.zeros(1025, 1), torch.zeros(1025, 1))):
        with pytest.raises(ValueError):
            compute_ot_plan(a, b)
    for plan, kw in ((torch.zeros(4, 5), {}), (torch.zeros(4), {}), (torch.zeros(0, 0), {}), (torch.zeros(1025, 1025), {}),
                     (torch.zeros(4, 4), dict(n_pairs=0)), (torch.zeros(4, 4), dict(n_pairs=65537)),
                     (torch.zeros(4, 4), dict(draw_index=-1)), (torch.zeros(4, 4), dict(draw_index=2 ** 32))):
        with pytest.raises(ValueError):
            sample_plan(plan, **kw)
    for reg in (0.0, -0.05, float("nan")):
        with pytest.raises(ValueError):
            OTPlanSampler("sinkhorn", reg=reg)
    with pytest.raises(ValueError):
        OTPlanSampler("emd")
    with pytest.raises(ValueError):
        OTPlanSampler("sinkhorn", draw_index=-1)
    with pytest.raises(ValueError):
        OTPlanSampler("exact").get_map(torch.zeros(4, 3), torch.zeros(5, 3))
    with pytest.raises(ValueError):
        compute_ot_pairing(x, x, method="pot")
    s = OTPlanSampler("sinkhorn", reg=0.1, normalize_cost=True, seed=9)
    assert (s.method, s.reg, s.normalize_cost, s.seed, s.draw_index) == ("sinkhorn", 0.1, True, 9, 0)
    assert s._next_draw() == 0 and s._next_draw() == 1 and s.state_dict() == {"seed": 9, "draw_index": 2}
    t = OTPlanSampler("sinkhorn")
    t.load_state_dict(s.state_dict())
    assert t._next_draw() == 2
    t.draw_index = 2 ** 32
    with pytest.raises(ValueError):
        t._next_draw()
    # an inpainting batch cannot be re-drawn row by row
    batch = ({"target_latents": torch.zeros(2, 4, 8, 8), "source_latents": torch.zeros(2, 4, 8, 8), "mask_pixels": torch.zeros(2, 1, 128, 128)},
             torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="sinkhorn_sample"):
        batch_to_data(batch, torch.device("cpu"), mask_encoder=lambda m: torch.zeros(2, 4, 8, 8), ot_method="sinkhorn_sample")
