"""The exact mini-batch OT pairing on the device (fc_ot_pairing_exact, fc_ot_assign) against the weak-duality certificate of
tests/ot_exact_ref.py -- g + B phi <= tau = B^3 2^-52 max(c) on the matrix the device wrote, a bound tests/test_ot_exact_cpu.py shows
the fp64 reference to meet on these same matrices -- plus the reference's permutation where ties decide, brute force for B <= 7,
the hazards (non-finite rows, batch range, repeat calls, the greedy path's bits around an exact call) and the training path.

Every entry of the cost matrix is held to 1e-6 relative of the fp64 squared distance; it is summed in fp32, up to 1024 terms to a
thread."""
import numpy as np
import pytest
import torch

import ot_exact_ref as R
from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _assign(c):
    from flocoder_amd._ops import ot_assign
    perm, duals = ot_assign(_dev(c))
    return perm.cpu().numpy(), duals[0].cpu().numpy(), duals[1].cpu().numpy()


def _certify(c, perm, u, v, tag):
    assert R.is_permutation(perm, c.shape[0]), tag
    gap, tau = R.certificate(c, perm, u, v)
    print(f"{tag}: g + B phi = {gap:.3e}, tau = {tau:.3e}")
    assert gap <= tau, (tag, gap, tau)


@pytest.mark.parametrize("case", R.PAIR_CASES)
def test_exact_pairing_meets_the_certificate(case):
    from flocoder_amd._ops import ot_pairing
    from flocoder_amd.ot import compute_ot_pairing_exact, pairing_cost
    B, D = case
    s, t = R.pair_case(B, D)
    sd, td = _dev(s), _dev(t)
    perm_d, info = compute_ot_pairing_exact(sd, td, return_info=True)
    assert perm_d.dtype == torch.int64 and perm_d.device.type == "cuda" and info["u"].dtype == torch.float64
    perm, c = perm_d.cpu().numpy(), info["cost"].cpu().numpy()
    ref = R.sqdist64(s, t)
    err = float((np.abs(c - ref)[ref > 0] / ref[ref > 0]).max())
    print(f"{case}: cost matrix max entrywise relative error {err:.3e}, rel-L2 {rel_l2(c, ref):.3e}")
    assert err < 1e-6
    _certify(c, perm, info["u"].cpu().numpy(), info["v"].cpu().numpy(), str(case))
    if B <= 7:
        assert R.perm_cost(c, perm) == R.brute_force(c)
    greedy, _ = ot_pairing(sd, td)
    ce, cg, ci = float(pairing_cost(sd, td, perm_d)), float(pairing_cost(sd, td, greedy)), float(pairing_cost(sd, td))
    print(f"{case}: pairing cost identity {ci:.4f}, greedy {cg:.4f}, exact {ce:.4f}")
    assert ce <= cg
    if case == (64, 1024):
        assert ce < cg and ce < ci
        assert R.perm_cost(c, perm) < R.perm_cost(c, greedy.cpu().numpy())
    assert torch.equal(compute_ot_pairing_exact(sd.view(B, 1, D), td.view(B, 1, D)), perm_d)       # any trailing shape, no info


@pytest.mark.parametrize("B,seed", R.TIE_CASES)
def test_assign_breaks_ties_as_the_reference(B, seed):
    c = R.tie_matrix(B, seed)
    perm, u, v = _assign(c)
    ref_perm, ref_u, ref_v = R.assign(c)
    assert np.array_equal(perm, ref_perm)
    assert np.array_equal(u, ref_u) and np.array_equal(v, ref_v)      # integer costs: every fp64 operation is exact
    _certify(c, perm, u, v, f"ties B={B}")


def test_assign_all_equal_is_the_identity():
    for B in (1, 70, 193):
        perm, u, v = _assign(R.equal_matrix(B))
        assert np.array_equal(perm, np.arange(B))
        _certify(R.equal_matrix(B), perm, u, v, f"equal B={B}")


def test_assign_reaches_the_optimum_where_the_greedy_sweep_cannot():
    from flocoder_amd import _binding as Bn
    c, best, greedy = R.greedy_trap()
    perm, u, v = _assign(c)
    assert R.perm_cost(c, perm) == best
    _certify(c, perm, u, v, "greedy trap")
    assert perm[0] == 1 and perm[1] == 0 and np.array_equal(perm[2:], np.arange(2, c.shape[0]))
    assert best < greedy
    # no duals asked for: the same permutation
    cd = _dev(c)
    p2 = torch.empty(c.shape[0], device=DEV, dtype=torch.int64)
    Bn.check(Bn.lib().fc_ot_assign(Bn.ptr(cd), c.shape[0], Bn.ptr(p2), None, Bn.current_stream(cd.device)))
    assert np.array_equal(p2.cpu().numpy(), perm)


def test_assign_largest_batch_meets_the_certificate():
    c = R.random_matrix(1024, 1024)
    perm, u, v = _assign(c)
    _certify(c, perm, u, v, "random B=1024")


@pytest.mark.parametrize("kind", ["both", "row", "col"])
def test_non_finite_rows_leave_a_permutation_and_an_optimal_finite_part(kind):
    """A NaN source row and an inf target row, together and each alone (alone, a finite row or column has to take a sentinel)."""
    from flocoder_amd.ot import compute_ot_pairing_exact
    s, t = R.hazard_case(kind)
    perm_d, info = compute_ot_pairing_exact(_dev(s), _dev(t), return_info=True)
    perm, c = perm_d.cpu().numpy(), info["cost"].cpu().numpy()
    assert R.is_permutation(perm, 70)
    assert np.isfinite(c).all()
    assert (c[5] == R.FLT_MAX).all() or kind == "col"
    assert (c[:, 40] == R.FLT_MAX).all() or kind == "row"
    sub, ident, us, vs = R.finite_part(c, perm, info["u"].cpu().numpy(), info["v"].cpu().numpy())
    assert sub.shape[0] >= 68 and sub.max() < R.FLT_MAX
    _certify(sub, ident, us, vs, f"finite part ({kind})")


def test_assign_cleans_raw_non_finite_entries():
    raw = R.hazard_raw()
    perm, u, v = _assign(raw)
    ref = R.assign(raw)
    assert R.is_permutation(perm, 70) and np.array_equal(perm, ref[0])
    sub, ident, us, vs = R.finite_part(raw, perm, u, v)
    _certify(sub, ident, us, vs, "finite part (raw)")


def test_batch_range_and_cpu_tensors():
    from flocoder_amd import _binding as Bn
    from flocoder_amd._ops import ot_assign, ot_pairing_exact
    from flocoder_amd.ot import compute_ot_pairing, compute_ot_pairing_exact
    for B in (0, 1025):
        with pytest.raises(ValueError):
            compute_ot_pairing_exact(torch.zeros(B, 4, device=DEV), torch.zeros(B, 4, device=DEV))
        with pytest.raises(ValueError):
            ot_assign(torch.zeros(B, B, device=DEV))
    z = torch.zeros(1025, 2, device=DEV)
    ws, p = torch.zeros(1025 * 1025, device=DEV), torch.zeros(1025, device=DEV, dtype=torch.int64)
    st = Bn.current_stream(z.device)
    assert Bn.lib().fc_ot_pairing_exact(Bn.ptr(z), Bn.ptr(z), 1025, 2, Bn.ptr(ws), Bn.ptr(p), None, st) == Bn.FC_E_SHAPE
    assert Bn.lib().fc_ot_assign(Bn.ptr(ws), 0, Bn.ptr(p), None, st) == Bn.FC_E_SHAPE
    assert Bn.lib().fc_ot_assign(None, 4, Bn.ptr(p), None, st) == Bn.FC_E_ARG
    assert Bn.lib().fc_ot_pairing_exact(Bn.ptr(z), Bn.ptr(z), 4, 2, None, Bn.ptr(p), None, st) == Bn.FC_E_ARG
    with pytest.raises(RuntimeError):
        compute_ot_pairing_exact(torch.zeros(4, 3), torch.zeros(4, 3))
    with pytest.raises(ValueError):
        compute_ot_pairing(z[:4], z[:4], method="pot")
    perm, cost, duals = ot_pairing_exact(z[:4], z[:4])
    assert perm.tolist() == [0, 1, 2, 3] and float(cost.abs().max()) == 0.0 and duals.shape == (2, 4)


def test_repeat_calls_agree_and_the_greedy_bits_stay():
    from flocoder_amd._ops import ot_pairing, ot_pairing_exact
    from oracle.synth import synth_input
    g = load_golden("g7_ot")
    gs = {B: (synth_input(f"g7.s{B}", (B, D), 7).to(DEV), synth_input(f"g7.t{B}", (B, D), 7).to(DEV)) for B, D in ((64, 64), (256, 1024))}
    before = {B: ot_pairing(*gs[B]) for B in gs}
    for B, D in ((64, 64), (256, 1024)):
        assert torch.equal(before[B][0].cpu(), torch.from_numpy(g[f"perm_{B}_{D}"]))
    s, t = (_dev(a) for a in R.pair_case(130, 37))
    a, b = ot_pairing_exact(s, t), ot_pairing_exact(s, t)       # back to back on one stream
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for B in gs:
        ot_pairing_exact(*gs[B])
        perm, dist = ot_pairing(*gs[B])
        assert torch.equal(perm, before[B][0]) and torch.equal(dist, before[B][1])


# ---- the training path --------------------------------------------------------------------------------------------------------
def _trainer(seed=0):
    from flocoder_amd.train import FlowTrainer
    from flocoder_amd.unet import Unet
    torch.manual_seed(seed)
    return FlowTrainer(Unet(dim=32, channels=4, dim_mults=(1, 2, 4, 8), n_classes=10).to(DEV).train(), lr=1e-3)


def _batch():
    g = torch.Generator().manual_seed(5)
    return torch.randn(16, 4, 8, 8, generator=g), torch.randn(16, 4, 8, 8, generator=g) * 0.7, torch.randint(0, 10, (16,), generator=g)


def test_step_with_the_exact_pairing_equals_step_on_gathered_targets():
    from flocoder_amd.ot import compute_ot_pairing, compute_ot_pairing_exact
    src, tgt, cls = (x.to(DEV) for x in _batch())
    u = torch.rand(16, generator=torch.Generator().manual_seed(6)).to(DEV)
    perm = compute_ot_pairing(src, tgt, method="exact")
    assert torch.equal(perm, compute_ot_pairing_exact(src, tgt)) and R.is_permutation(perm.cpu().numpy(), 16)
    a, b = _trainer(), _trainer()
    assert torch.equal(a.params, b.params)
    la = a.step(src, tgt, {"class_cond": cls}, u=u, pairing=perm)
    lb = b.step(src, tgt[perm].contiguous(), {"class_cond": cls}, u=u)
    assert float(la) == float(lb) and torch.equal(a.params, b.params)


def test_batch_to_data_and_train_batch_take_the_method():
    from flocoder_amd.ot import compute_ot_pairing
    from flocoder_amd.train import batch_to_data
    _, lat, cls = _batch()
    torch.manual_seed(3)
    src, tgt, _, _, _ = batch_to_data((lat, cls), torch.device(DEV), ot_method="exact")
    torch.manual_seed(3)
    noise = torch.randn_like(lat.to(DEV))
    assert torch.equal(src, noise)
    assert torch.equal(tgt, lat.to(DEV)[compute_ot_pairing(noise, lat.to(DEV), method="exact")])
    with pytest.raises(ValueError):
        batch_to_data((lat, cls), torch.device(DEV), ot_method="hungarian")
    # train_batch: the default is the greedy pairing, bit for bit; "exact" is step fed the exact pairing
    for method in ("greedy", "exact"):
        a, b = _trainer(1), _trainer(1)
        torch.manual_seed(4)
        la = a.train_batch((lat, cls), cfg_drop=0.0) if method == "greedy" else a.train_batch((lat, cls), cfg_drop=0.0, ot_method="exact")
        torch.manual_seed(4)
        target = lat.to(DEV)
        noise = torch.randn_like(target)
        perm = compute_ot_pairing(noise, target) if method == "greedy" else compute_ot_pairing(noise, target, method="exact")
        lb = b.step(noise, target[perm], {"class_cond": cls.to(DEV), "mask_cond": None})
        assert float(la) == float(lb) and torch.equal(a.params, b.params), method
