"""The exact OT pairing's reference (tests/ot_exact_ref.py) against brute force and scipy, and the certificate bound shown on the CPU to
be one the reference itself meets on every matrix the GPU tests use (tests/test_gpu_ot_exact.py imports the same generators)."""
import numpy as np
import pytest

import ot_exact_ref as R


def _small_matrices(B):
    g = np.random.default_rng(B)
    yield g.random((B, B), dtype=np.float32) * 10
    yield (g.standard_normal((B, B)) * 100).astype(np.float32)         # negative entries too
    yield R.tie_matrix(B, 10 + B)
    yield g.integers(0, 2, size=(B, B)).astype(np.float32)
    yield R.equal_matrix(B)


@pytest.mark.parametrize("B", range(1, 8))
def test_ref_matches_brute_force(B):
    for c in _small_matrices(B):
        perm, u, v = R.assign(c)
        assert R.is_permutation(perm, B)
        assert R.perm_cost(c, perm) == pytest.approx(R.brute_force(c), rel=1e-12, abs=1e-12)
        gap, tau = R.certificate(c, perm, u, v)
        assert gap <= tau, (gap, tau)


def test_ref_all_equal_is_identity_and_ties_go_low():
    for B in (1, 5, 70):
        assert np.array_equal(R.assign(R.equal_matrix(B))[0], np.arange(B))
    perm, _, _ = R.assign(np.array([[1, 1, 5], [1, 1, 5], [5, 5, 5]], dtype=np.float32))
    assert perm.tolist() == [0, 1, 2]


def test_ref_cost_equals_scipy():
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    mats = [R.tie_matrix(B, s) for B, s in R.TIE_CASES] + [R.random_matrix(B, B) for B in (3, 64, 65, 193, 300)] + [R.greedy_trap()[0]]
    mats += [R.sqdist32(*R.pair_case(B, D)) for B, D in R.PAIR_CASES if B <= 200]
    for c in mats:
        perm, _, _ = R.assign(c)
        rows, cols = lsa(c.astype(np.float64))
        want = float(c.astype(np.float64)[rows, cols].sum())
        assert R.perm_cost(c, perm) == pytest.approx(want, rel=1e-12, abs=1e-12)


@pytest.mark.parametrize("case", R.PAIR_CASES)
def test_certificate_holds_for_the_ref_on_the_pairing_cases(case):
    c = R.sqdist32(*R.pair_case(*case))
    perm, u, v = R.assign(c)
    assert R.is_permutation(perm, case[0])
    gap, tau = R.certificate(c, perm, u, v)
    print(f"{case}: g + B phi = {gap:.3e}, tau = {tau:.3e}")
    assert gap <= tau, (gap, tau)


def test_certificate_holds_for_the_ref_on_the_handcrafted_matrices():
    mats = [R.tie_matrix(B, s) for B, s in R.TIE_CASES] + [R.equal_matrix(B) for B in (1, 70, 193)]
    mats += [R.greedy_trap()[0], R.random_matrix(1024, 1024)]
    for c in mats:
        perm, u, v = R.assign(c)
        assert R.is_permutation(perm, c.shape[0])
        gap, tau = R.certificate(c, perm, u, v)
        print(f"B = {c.shape[0]}: g + B phi = {gap:.3e}, tau = {tau:.3e}")
        assert gap <= tau, (gap, tau)
    c, best, greedy = R.greedy_trap()
    assert R.perm_cost(c, R.assign(c)[0]) == best < greedy


def test_certificate_rejects_duals_out_of_the_costs_scale():
    c = R.random_matrix(8, 8)
    perm, u, v = R.assign(c)
    assert R.certificate(c, perm, u, v)[0] == 0.0
    worse = np.roll(perm, 1)
    assert R.certificate(c, worse, u, v)[0] > R.certificate(c, worse, u, v)[1]
    gap, tau = R.certificate(c, worse, u + R.FLT_MAX, v - R.FLT_MAX)       # every cost absorbed: g and phi would both read 0
    assert gap > tau


@pytest.mark.parametrize("kind", ["both", "row", "col", "raw"])
def test_certificate_holds_on_the_finite_part_of_the_hazard_cases(kind):
    c = R.hazard_raw() if kind == "raw" else R.sqdist32(*R.hazard_case(kind))
    c = R.clean(c)
    assert np.isfinite(c).all()
    assert (c[5] == R.FLT_MAX).all() or kind == "col"
    assert (c[:, 40] == R.FLT_MAX).all() or kind == "row"
    perm, u, v = R.assign(c)
    assert R.is_permutation(perm, 70)
    sub, ident, us, vs = R.finite_part(c, perm, u, v)
    assert sub.shape[0] >= 68 and (sub.max() < R.FLT_MAX or kind == "raw")
    gap, tau = R.certificate(sub, ident, us, vs)
    print(f"hazard: g + B phi = {gap:.3e}, tau = {tau:.3e}")
    assert gap <= tau, (gap, tau)
    assert R.perm_cost(sub, ident) == pytest.approx(R.perm_cost(sub, R.assign(sub)[0]), rel=1e-12)


def test_python_surface_rejects_what_it_cannot_run():
    import torch
    from flocoder_amd.ot import compute_ot_pairing, compute_ot_pairing_exact
    s, t = torch.zeros(4, 3), torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        compute_ot_pairing_exact(s, t)
    with pytest.raises(RuntimeError, match="no CPU path"):
        compute_ot_pairing(s, t, method="exact")
    with pytest.raises(ValueError, match="greedy"):
        compute_ot_pairing(s, t, method="sinkhorn")
