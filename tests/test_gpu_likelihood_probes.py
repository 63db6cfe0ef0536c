"""K Hutchinson probes in one likelihood solve and the counter-based probe field on the GPU (fc_unet_log_likelihood_probes,
fc_unet_log_likelihood_rk45_probes, fc_ode_probe_field).  Almost every check is an equality of bits against the single-probe entry
points, which tests/test_gpu_likelihood.py and tests/test_gpu_likelihood_rk45.py gate against the fp64 restatements; the distinct-probe
adaptive solve is held to the golden that tools/make_ll_probes_golden.py wrote (tests/likelihood_probes_ref.py), with the gates and
constants of tests/test_gpu_likelihood_rk45.py, the Cauchy-Schwarz term averaged over the probes because a is the integral of their mean.

Cases:  A  d16c10, class ids, B = 2, 16x16 (m = 1024: exactly one trip of the 256 x 4 loop)
        B  dim 8, mask-conditioned, B = 2, 8x8 (m = 256: three quarters of the workgroup idle; the whole-network-per-sample plan)
        C  d32c102, class ids, 5 rows of a plan reserved for 8, 32x32 (m = 4096: four trips; B < maxB, where a mixed stride goes wrong)
A and B are the golden's cases (likelihood_probes_ref.case_inputs); RK4 grids have 5 points (9 for A).  With -s the golden test prints
its figures.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import likelihood_probes_ref as pr
import test_gpu_likelihood_rk45 as t45
from conftest import load_golden, rel_l2
from oracle.synth import synth_input, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G_TOL, TRAJ_TOL, NFEV_SLACK = t45.G_TOL, t45.TRAJ_TOL, t45.NFEV_SLACK
RK4_POINTS = {"A": 9, "B": 5, "C": 5}
GOLDEN_ID = {"A": "d16c10-class", "B": "d8mask"}
_IN, _RK4 = {}, {}


def _inputs(case):
    """(state dict, x, eps [3, B, ...], cond, rows to reserve before the call or 0), made once"""
    if case not in _IN:
        if case in GOLDEN_ID:
            _IN[case] = pr.case_inputs(GOLDEN_ID[case]) + (0,)
        else:
            sd = synth_state_dict(load_golden("g3_unet_d32c102")["shapes"], 1)
            x = synth_input("llp.x.C", (5, 4, 32, 32), 1)
            eps = torch.stack([torch.where(synth_input(f"llp.eps.C{k}", (5, 4, 32, 32), 1) >= 0, 1.0, -1.0) for k in range(3)])
            cond = {"class_cond": torch.randint(0, 102, (5,), generator=torch.Generator().manual_seed(3001))}
            _IN[case] = (sd, x, eps, cond, 8)
    return _IN[case]


def _model(case, train=False):
    sd, x, _, _, reserve = _inputs(case)
    model = t45._model(sd, train)
    if reserve:        # a training-form plan for more rows than the call brings
        model._forward_native(torch.zeros(reserve, 4, x.shape[-1], x.shape[-1], device=DEV), torch.zeros(reserve, device=DEV), None, None, train=True)
    return model


def _kw(cond):
    from flocoder_amd.sampling import _mask_flags
    dc = t45._dcond(cond) or {}
    mask, ones = _mask_flags(dc)
    return dict(class_ids=dc.get("class_cond"), mask=mask, mask_is_ones=ones)


def _rk4(model, x, eps, cond, n, **kw):
    """Unet.log_likelihood on the reversed grid: (z, a, logp[, a_probes, stderr]) on the host"""
    from flocoder_amd import sampling as S
    z = x.to(DEV).contiguous().clone()
    out = model.log_likelihood(z, S.rk4_time_grid(n).flip(0), eps.to(DEV).contiguous(), **_kw(cond), **kw)
    torch.cuda.synchronize()
    return (z.cpu(),) + tuple(o.cpu() for o in out)


def _rk45(model, x, eps, cond, per_sample, **kw):
    """Unet.log_likelihood_rk45: (z, a, logp, counters [G, 3][, a_probes, stderr]) on the host"""
    z = x.to(DEV).contiguous().clone()
    c, a, logp, *extra = model.log_likelihood_rk45(z, eps.to(DEV).contiguous(), per_sample=per_sample, **_kw(cond), **kw)
    torch.cuda.synchronize()
    counts = torch.stack(list(c), 1) if per_sample else torch.tensor([list(c)])
    return (z.cpu(), a.cpu(), logp.cpu(), counts) + tuple(e.cpu() for e in extra)


def _rk4_runs(case):
    """One model per case, training form kept: the K = 3 call twice, the three single-probe calls, the K = 1 call of the new entry point"""
    if case not in _RK4:
        _, x, eps, cond, _ = _inputs(case)
        model, n = _model(case), RK4_POINTS[case]
        run = lambda e: _rk4(model, x, e, cond, n, restore_plan=False)
        _RK4[case] = dict(k3=run(eps), single=[run(eps[k]) for k in range(3)], k1=run(eps[:1]), k3_again=run(eps))
    return _RK4[case]


def _stderr(a_probes, a):
    k = a_probes.shape[0]
    return torch.sqrt(((a_probes - a) ** 2).sum(0) / (k * (k - 1)))


@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_rk4_every_probe_has_the_bits_of_its_single_probe_call(case):
    r = _rk4_runs(case)
    z, a, logp, a_probes, se = r["k3"]
    assert a_probes.shape == (3, z.shape[0]) and a_probes.dtype == torch.float64 and torch.isfinite(a_probes).all()
    for k in range(3):
        zk, ak, _ = r["single"][k]
        assert torch.equal(z, zk), k
        assert torch.equal(a_probes[k], ak), (k, a_probes[k].tolist(), ak.tolist())
    assert not torch.equal(a_probes[0], a_probes[1])            # (the probes are distinct: the equalities above are not vacuous)


@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_rk4_one_probe_through_the_new_entry_point_and_repeats(case):
    r = _rk4_runs(case)
    z1, a1, logp1, ap1, se1 = r["k1"]
    z0, a0, logp0 = r["single"][0]
    assert torch.equal(a1, a0) and torch.equal(logp1, logp0) and torch.equal(z1, z0) and torch.equal(ap1[0], a0)
    assert bool(torch.isnan(se1).all())
    assert all(torch.equal(p, q) for p, q in zip(r["k3"], r["k3_again"]))


@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_rk4_mean_logp_and_standard_error(case):
    z, a, logp, a_probes, se = _rk4_runs(case)["k3"]
    mean = (a_probes[0] + a_probes[1] + a_probes[2]) / 3
    assert torch.equal(a, mean)
    D = z[0].numel()
    # the existing formula as ode_ll_logp_kernel forms it: (-|z|^2/2 - (D/2) ln 2pi) + a, the norm summed by the library for a = 0
    base = _rk4_runs(case)["single"][0]
    assert torch.equal(logp, (base[2] - base[1]) + a) or float((logp - (-0.5 * z.double().flatten(1).pow(2).sum(1) - 0.5 * D * math.log(2 * math.pi) + a)).abs().max()) <= 1e-12 * float(logp.abs().max())
    assert float((logp - (-0.5 * z.double().flatten(1).pow(2).sum(1) - 0.5 * D * math.log(2 * math.pi) + a)).abs().max()) <= 1e-12 * float(logp.abs().max())
    ref = _stderr(a_probes, a)
    assert bool(((se - ref).abs() <= 1e-14 * ref).all()), (se.tolist(), ref.tolist())
    assert bool((se > 0).all())


@pytest.mark.parametrize("mode", ["ps", "coupled"])
@pytest.mark.parametrize("case", ["A", "B"])
def test_rk45_copies_of_one_probe_are_the_single_probe_solve(case, mode):
    _, x, eps, cond, _ = _inputs(case)
    model = _model(case)
    ps = mode == "ps"
    z0, a0, logp0, c0 = _rk45(model, x, eps[0], cond, ps, restore_plan=False)
    assert bool((c0[:, 2] >= 1).all())
    for k in (2, 4):
        z, a, logp, c, a_probes, se = _rk45(model, x, eps[:1].expand(k, *x.shape).contiguous(), cond, ps, restore_plan=False)
        assert torch.equal(c, c0), (k, c.tolist(), c0.tolist())
        assert torch.equal(z, z0) and torch.equal(a, a0) and torch.equal(logp, logp0), k
        for j in range(k):
            assert torch.equal(a_probes[j], a), (k, j, a_probes[j].tolist(), a.tolist())
        assert bool((se == 0.0).all()), (k, se.tolist())


@pytest.mark.parametrize("mode", ["ps", "coupled"])
@pytest.mark.parametrize("case", ["A", "B"])
def test_rk45_distinct_probes_against_the_scipy_golden(case, mode):
    cid = GOLDEN_ID[case]
    g = load_golden("ll_probes_rk45_scipy_oracle")
    _, x, eps, cond, _ = _inputs(case)
    ref = {k: g[f"{cid}.{mode}.{k}"] for k in ("z", "a", "logp", "counts", "gsum", "a_probes")}
    assert (ref["counts"][:, 2] >= 1).all()
    model = _model(case)
    ps = mode == "ps"
    r1 = _rk45(model, x, eps, cond, ps, restore_plan=False)
    r2 = _rk45(model, x, eps, cond, ps, restore_plan=False)
    z, a, logp, counts, a_probes, se = r1
    assert torch.equal(counts, r2[3]) and torch.equal(z, r2[0]) and torch.equal(a, r2[1])
    dev = (a_probes.mean(0) - a).abs()
    lim = 1e-11 * (1 + a_probes.abs().max(0).values)
    zr = torch.from_numpy(ref["z"])
    en = eps.double().flatten(2).norm(dim=2)                                               # [K, B]
    bound = G_TOL * (en * torch.from_numpy(ref["gsum"])).mean(0) + 2 * torch.from_numpy(np.abs(ref["a"] - g[f"{cid}.a_tight"]))
    ratio = (a - torch.from_numpy(ref["a"])).abs() / bound
    zerr = [rel_l2(z[b], zr[b]) for b in range(x.shape[0])]
    print(f"\n[{case} {mode}] counters {counts.tolist()} (scipy {ref['counts'].tolist()}); z rel-L2 {zerr}; a_gpu {a.tolist()}, a_ref {ref['a'].tolist()}, "
          f"bound {bound.tolist()}, |a_gpu - a_ref| / bound {ratio.tolist()}; |mean_k a_k - a| {dev.tolist()} (limit {lim.tolist()}); "
          f"a_probes {a_probes.tolist()} (scipy {ref['a_probes'].tolist()}); stderr {se.tolist()}")
    assert bool((dev <= lim).all()), (dev.tolist(), lim.tolist())
    assert bool(((counts[:, 0] - torch.from_numpy(ref["counts"][:, 0])).abs() <= NFEV_SLACK).all()), (counts.tolist(), ref["counts"].tolist())
    assert max(zerr) < TRAJ_TOL, zerr
    assert bool((ratio <= 1).all()), ratio
    ref_se = _stderr(a_probes, a)
    assert bool(((se - ref_se).abs() <= 1e-14 * ref_se).all())


def test_rk45_constant_field_with_three_probes():
    """v = c, g = 0: a, every a_k and the standard error are exactly 0.0 and the counters are scipy's on the augmented system."""
    m, c, x = t45._const_model()
    eps = torch.stack([torch.where(torch.randn(x.shape, generator=torch.Generator().manual_seed(5 + k)) >= 0, 1.0, -1.0) for k in range(3)])
    cfull = c.view(4, 1, 1).expand(4, 16, 16).double().numpy().reshape(-1)
    aug = lambda rows: (lambda t, y: np.concatenate([np.tile(cfull, rows), np.zeros(rows)]))
    y0 = lambda xs: np.concatenate([xs.double().numpy().reshape(-1), np.zeros(xs.shape[0])])
    refs = {True: [t45._scipy_counts(aug(1), y0(x[b:b + 1])) for b in range(2)], False: [t45._scipy_counts(aug(2), y0(x))]}
    for ps in (True, False):
        z, a, logp, counts, a_probes, se = _rk45(m, x, eps, None, ps, restore_plan=False)
        assert counts.tolist() == refs[ps], (counts.tolist(), refs[ps])
        assert bool((a == 0.0).all()) and bool((a_probes == 0.0).all()) and bool((se == 0.0).all())
        assert not bool(torch.signbit(a).any())


def _device_field(kind, seed, probe, ids, per):
    from flocoder_amd import sampling as S
    out = S.probe_field(seed, probe, torch.tensor(ids, dtype=torch.int64), (len(ids), per), kind, DEV)
    torch.cuda.synchronize()
    return out.cpu()


def test_rademacher_probe_field_is_the_numpy_form_bit_for_bit():
    from flocoder_amd import noise as N
    ids = [7, 0, 2 ** 33 + 1]
    for per in (256, 4096):
        for probe in (0, 5):
            got = _device_field("rademacher", 3, probe, ids, per)
            ref = torch.from_numpy(N.probe_field(3, probe, ids, per, "rademacher"))
            assert got.dtype == torch.float32 and torch.equal(got, ref), (per, probe)
            assert bool((got.abs() == 1.0).all())
            assert torch.equal(_device_field("rademacher", 3, probe, [7], per)[0], got[0])       # id 7 alone and as row 0 of three
    f = _device_field("rademacher", 3, 0, ids, 4096)
    assert abs(float(f.double().mean())) <= 5 / math.sqrt(f.numel())
    assert not torch.equal(_device_field("rademacher", 3, 5, ids, 4096), f) and not torch.equal(_device_field("rademacher", 4, 0, ids, 4096), f)


def test_gaussian_probe_field_is_the_numpy_form_bit_for_bit():
    """The Gaussian kind evaluates the normal field's transform in fp64 and rounds once, on the device as in NumPy: equal bits, the
    sampler's tail cut, and -- the uniforms being the sampler's -- values within the rounding of that field's fp32 transform of
    fc_ode_normal_field under the same key (the gate of tests/test_gpu_sde.py, against the fp64 value)."""
    from flocoder_amd import noise as N
    from flocoder_amd import sampling as S
    ids = [7, 0, 2 ** 33 + 1]
    key = (3 + N.PROBE_KEY_OFFSET) & 0xffffffffffffffff
    for per in (256, 4096):
        for probe in (0, 5):
            got = _device_field("gaussian", 3, probe, ids, per)
            ref = torch.from_numpy(N.probe_field(3, probe, ids, per, "gaussian"))
            frac = float((got == ref).float().mean())
            print(f"\ngaussian probe field per={per} probe={probe}: {frac:.6f} of the entries bit-equal")
            assert got.dtype == torch.float32 and torch.equal(got, ref), (per, probe, frac)
            assert torch.equal(_device_field("gaussian", 3, probe, [7], per)[0], got[0])
            assert float(got.abs().max()) <= N.TAIL
            sde = S.normal_field(key, probe, torch.tensor(ids), (3, per), DEV).cpu()
            ref64 = torch.from_numpy(N.normal_field(key, probe, ids, per))
            assert bool(((sde.double() - ref64).abs() <= 6 * 2.0 ** -24 * ref64.abs()).all())
    f = _device_field("gaussian", 3, 0, ids, 4096).double()
    assert abs(float(f.mean())) <= 5 / math.sqrt(f.numel()) and abs(float(f.pow(2).mean()) - 1) <= 5 * math.sqrt(2 / f.numel())


@pytest.mark.parametrize("method", ["rk45", "rk4"])
def test_a_samples_likelihood_does_not_depend_on_its_batch(method):
    from flocoder_amd import sampling as S
    sd, x, _, cond, _ = _inputs("A")
    gen = torch.Generator().manual_seed(91)
    x3 = torch.cat([2.0 * torch.randn(1, *x.shape[1:], generator=gen), x[:1], 2.0 * torch.randn(1, *x.shape[1:], generator=gen)])
    c3 = torch.cat([torch.tensor([0]), cond["class_cond"][:1], torch.tensor([9])])
    kw = dict(method=method, n_steps=9, n_probes=2, probe_seed=3, per_sample=True, return_info=True)
    model = t45._model(sd)
    lp1, z1, nfe1, i1 = S.log_likelihood(model, x3[1:2].to(DEV), cond={"class_cond": c3[1:2].to(DEV)}, sample_ids=[5], **kw)
    lp3, z3, nfe3, i3 = S.log_likelihood(model, x3.to(DEV), cond={"class_cond": c3.to(DEV)}, sample_ids=[9, 5, 4], **kw)
    torch.cuda.synchronize()
    assert i1["n_probes"] == 2 and i3["a_probes"].shape == (2, 3)
    assert torch.equal(lp3[1:2], lp1) and torch.equal(i3["logp_stderr"][1:2], i1["logp_stderr"]) and torch.equal(z3[1:2], z1)
    assert torch.equal(i3["a_probes"][:, 1:2], i1["a_probes"])
    if method == "rk45":      # the sample's own counters
        e1 = torch.stack([S.probe_field(3, k, [5], x3[1:2].shape, device=DEV) for k in range(2)])
        e3 = torch.stack([S.probe_field(3, k, [9, 5, 4], x3.shape, device=DEV) for k in range(2)])
        assert torch.equal(e3[:, 1:2], e1)
        n1 = _rk45(model, x3[1:2], e1, {"class_cond": c3[1:2]}, True)[3]
        n3 = _rk45(model, x3, e3, {"class_cond": c3}, True)[3]
        assert torch.equal(n3[1:2], n1) and nfe1 == int(n1[:, 0].max())


@pytest.mark.timeout(600)
def test_a_k_probe_call_leaks_nothing():
    from flocoder_amd import _binding as B
    from flocoder_amd import sampling as S
    from flocoder_amd.train import FlowTrainer
    gd = load_golden("g10_train_step")
    sd = synth_state_dict(gd["shapes"], 10)
    cls = torch.from_numpy(gd["cls"]).to(DEV)[:4]
    xl = (0.2 * synth_input("llp.hyg.x", (4, 4, 16, 16), 1)).to(DEV)
    el = torch.stack([torch.where(synth_input(f"llp.hyg.e{k}", (4, 4, 16, 16), 1) >= 0, 1.0, -1.0) for k in range(3)]).to(DEV)
    src = synth_input("llp.hyg.src", (4, 4, 16, 16), 2).to(DEV)
    cond = {"class_cond": cls}
    short = dict(method="rk45", rtol=1e-2, atol=1e-2)

    def calls(m):
        out = [S.generate_latents_rk4(m, (4, 4, 16, 16), 4, cond, 3.0, source=src)[0],
               S.log_likelihood(m, xl, n_steps=3, cond=cond, probe=el[0])[0],
               S.log_likelihood(m, xl, cond=cond, probe=el[0], **short)[0]]
        torch.cuda.synchronize()
        return [o.clone() for o in out]

    def k3(m, **kw):
        out = [S.log_likelihood(m, xl, n_steps=3, cond=cond, probe=el, return_info=True, **kw),
               S.log_likelihood(m, xl, cond=cond, probe=el, return_info=True, **short, **kw)]
        torch.cuda.synchronize()
        return [t.clone() for r in out for t in (r[0], r[1], r[3]["a_probes"], r[3]["logp_stderr"])]

    def ll1(m):
        out = [S.log_likelihood(m, xl, n_steps=3, cond=cond, probe=el[0])[0], S.log_likelihood(m, xl, cond=cond, probe=el[0], **short)[0]]
        torch.cuda.synchronize()
        return [o.clone() for o in out]

    same = lambda p, q: [torch.equal(u, v) for u, v in zip(p, q)]
    used, fresh = t45._model(sd), t45._model(sd)
    before = calls(used)
    k3(used)
    assert B.lib().fc_unet_train_form(used._handle) == 0
    sampler_after = S.generate_latents_rk4(used, (4, 4, 16, 16), 4, cond, 3.0, source=src)[0]
    assert torch.equal(sampler_after, S.generate_latents_rk4(fresh, (4, 4, 16, 16), 4, cond, 3.0, source=src)[0])
    assert used.launches_per_forward == fresh.launches_per_forward
    after = calls(used)
    assert all(same(before, after)), same(before, after)
    # the two orders on models that ran nothing else (so both hold the reservation the call itself makes): K = 3 behind K = 1 -- the
    # buffers grow -- against K = 3 first, and K = 1 behind K = 3 against K = 1 first
    m1, m3 = t45._model(sd), t45._model(sd)
    one_first, three_first = ll1(m1), k3(m3)
    three_behind, one_behind = k3(m1), ll1(m3)
    assert all(same(three_behind, three_first)), same(three_behind, three_first)
    assert all(same(one_behind, one_first)), same(one_behind, one_first)

    def run(with_ll):
        from flocoder_amd.unet import Unet
        m = Unet(dim=16, channels=4, dim_mults=(1, 2, 4, 8), n_classes=10)
        m.load_state_dict(sd)
        tr = FlowTrainer(m.to(DEV).train(), lr=1e-4)
        out = []
        for step in (1, 2):
            s_, t_ = synth_input(f"g10.src{step}", (8, 4, 16, 16), 10), synth_input(f"g10.tgt{step}", (8, 4, 16, 16), 10)
            u = torch.sigmoid(synth_input(f"g10.u{step}", (8,), 10, scale=1.5))
            loss = tr.step(s_.to(DEV), t_.to(DEV), {"class_cond": torch.from_numpy(gd["cls"]).to(DEV), "mask_cond": None}, u=u.to(DEV))
            out.append((loss.clone(), tr.grads.clone(), tr.params.clone()))
            if with_ll and step == 1:
                assert all(torch.isfinite(t).all() for t in k3(m)) and m.training
        torch.cuda.synchronize()
        return out

    for (l0, g0, p0), (l1, g1, p1) in zip(run(False), run(True)):
        assert torch.equal(l0, l1) and torch.equal(g0, g1) and torch.equal(p0, p1)


def test_refusals():
    from flocoder_amd import _binding as B
    from flocoder_amd import sampling as S
    sd, x, eps, cond, _ = _inputs("A")
    model = t45._model(sd)
    xd, ed, cd = x.to(DEV), eps.to(DEV), t45._dcond(cond)
    cap = B.FC_LL_MAX_PROBES
    assert cap >= 64
    for k in (0, cap + 1):
        with pytest.raises(ValueError, match=str(cap)):
            S.log_likelihood(model, xd, cond=cd, n_probes=k)
        with pytest.raises(ValueError, match=str(cap)):
            model.log_likelihood(xd.clone(), S.rk4_time_grid(3).flip(0), ed[:1].expand(k, *x.shape).contiguous(), class_ids=cd["class_cond"])
        with pytest.raises(ValueError, match=str(cap)):
            model.log_likelihood_rk45(xd.clone(), ed[:1].expand(k, *x.shape).contiguous(), class_ids=cd["class_cond"])
    # the library itself refuses them, naming the cap
    model.log_likelihood(xd.clone(), S.rk4_time_grid(3).flip(0), ed, class_ids=cd["class_cond"], restore_plan=False)
    big = ed[:1].expand(cap + 1, *x.shape).contiguous()
    a, logp, se = (torch.empty(2, dtype=torch.float64, device=DEV) for _ in range(3))
    ap = torch.empty(cap + 1, 2, dtype=torch.float64, device=DEV)
    ts = S.rk4_time_grid(3).flip(0).float().contiguous()
    tp = ts.numpy().ctypes.data_as(C.POINTER(C.c_float))
    counters = (C.c_int * 6)()
    for k in (0, cap + 1):
        with pytest.raises(ValueError, match=str(cap)):
            B.check(B.lib().fc_unet_log_likelihood_probes(model._handle, B.ptr(xd.clone()), 2, 16, 16, tp, 3, 999.0, B.ptr(cd["class_cond"]), None, 0,
                                                          B.ptr(big), k, B.ptr(a), B.ptr(logp), B.ptr(ap), B.ptr(se), B.current_stream(xd.device)))
        with pytest.raises(ValueError, match=str(cap)):
            B.check(B.lib().fc_unet_log_likelihood_rk45_probes(model._handle, B.ptr(xd.clone()), 2, 16, 16, 1.0, 0.0, 1e-5, 1e-5, 999.0,
                                                               B.ptr(cd["class_cond"]), None, 0, B.ptr(big), k, 1, B.ptr(a), B.ptr(logp), B.ptr(ap),
                                                               B.ptr(se), counters, B.current_stream(xd.device)))
    model.release_training_plan()
    with pytest.raises(ValueError, match="n_probes"):
        S.log_likelihood(model, xd, cond=cd, probe=ed, n_probes=2)
    with pytest.raises(ValueError, match="generator"):
        S.log_likelihood(model, xd, cond=cd, probe_seed=1, generator=torch.Generator(device=DEV).manual_seed(1))
    with pytest.raises(ValueError, match="probe_seed"):
        S.log_likelihood(model, xd, cond=cd, sample_ids=[0, 1])
    for method in ("rk4", "rk45"):
        with pytest.raises(RuntimeError, match="no CPU path"):
            S.log_likelihood(model, x, cond=cond, n_probes=3, method=method)
    with pytest.raises(RuntimeError):
        model.log_likelihood_rk45(x.clone(), eps)
    # a K-probe call through the public function with drawn probes: the first draw is the K = 1 call's
    g = lambda: torch.Generator(device=DEV).manual_seed(1)
    lp1, _, _, i1 = S.log_likelihood(model, xd, n_steps=3, cond=cd, generator=g(), return_info=True)
    lp2, _, nfe, i2 = S.log_likelihood(model, xd, n_steps=3, cond=cd, generator=g(), n_probes=2, return_info=True)
    assert nfe == 8 and torch.equal(i2["a_probes"][0], i1["a"]) and i1["n_probes"] == 1 and bool(torch.isnan(i1["logp_stderr"]).all())
    assert B.lib().fc_unet_train_form(model._handle) == 0 and torch.equal(xd.cpu(), x)
