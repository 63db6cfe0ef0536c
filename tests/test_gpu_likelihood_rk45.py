"""The adaptive (RK45) flow log-likelihood and inversion on the GPU (fc_unet_log_likelihood_rk45; sampling.log_likelihood /
invert_latents with method="rk45") against scipy: exactly on a constant field, and on real fields against the golden that
tools/make_ll_rk45_golden.py wrote from tests/likelihood_rk45_ref.py (scipy's RK45 on [x, a] around the fp64 oracle U-Net).  The GPU
tests read the golden and never solve over the oracle themselves.

Gates, none of them measured on the code under test (per sample):
  z      relative L2 < TRAJ_TOL = 2e-4 and |nfev - ref| <= NFEV_SLACK = 12: the gates of tests/test_gpu_rk45.py, for its reasons
  a      |a_gpu - a_ref| <= G_TOL |eps_b| gsum_b + 2 |a_ref - a_tight|_b.  First term: the backward's per-sample d(x) gate (G_TOL = 2e-6,
         tests/unet_grad_taps.py) through Cauchy-Schwarz over the golden's own accepted steps, as tests/test_gpu_likelihood.py.  Second:
         two solves that may take an accept / reject decision differently are each only within the solver's error of the truth (triangle
         inequality); the figure is the golden's own -- its solve against its solve at the tight tolerance -- never the device's
  logp   that bound plus | |z_gpu|^2 - |z_ref|^2 | / 2
With -s every case prints its figures.

The fixtures are admitted on the oracle alone (tests/likelihood_rk45_ref.py, FP32_AGREEMENT): z of these solves moves by 1e-7 .. 3e-3
with the precision of the evaluations, so only cases whose fp32-oracle solve agrees with the fp64 one to a quarter of TRAJ_TOL are used.

Measured on the MI355X (worst sample per case; DESIGN.md section 4 has the table): counters equal to scipy's in all four cases; z rel-L2
d16c10 per sample 6.0e-6, coupled 2.3e-5, d8mask per sample 9.8e-6, coupled 3.3e-6; |a_gpu - a_ref| / bound at most 0.065, logp 0.065.
"""
import math

import numpy as np
import pytest
import torch

import likelihood_rk45_ref as rr
from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G_TOL, TRAJ_TOL, NFEV_SLACK = 2e-6, 2e-4, 12
_CASE = {}


def _model(sd, train=False):
    from flocoder_amd.unet import Unet
    from oracle import flow_oracle as fo
    m = fo.unet_meta(sd)
    model = Unet(dim=m["dim"], dim_mults=(1, 2, 4, 8), channels=4, n_classes=m["n_classes"], mask_cond=m["mask_cond"])
    model.load_state_dict(sd, strict=True)
    return model.to(DEV).train(train)


def _case(cid):
    """(state dict, x, eps, cond) of a golden case, made once."""
    if cid not in _CASE:
        _CASE[cid] = rr.case_inputs(cid)
    return _CASE[cid]


def _dcond(cond):
    return None if cond is None else {k: v.to(DEV) for k, v in cond.items()}


def _solve(model, x, eps, cond, per_sample, **kw):
    """Unet.log_likelihood_rk45 as sampling.log_likelihood drives it: (z, a, logp on the host, counters [G, 3])."""
    from flocoder_amd.sampling import _mask_flags
    dc = _dcond(cond) or {}
    mask, ones = _mask_flags(dc)
    z = x.to(DEV).contiguous().clone()
    c, a, logp = model.log_likelihood_rk45(z, eps.to(DEV).contiguous(), per_sample=per_sample, class_ids=dc.get("class_cond"), mask=mask,
                                           mask_is_ones=ones, **kw)
    torch.cuda.synchronize()
    counts = torch.stack(list(c), 1) if per_sample else torch.tensor([list(c)])
    return z.cpu(), a.cpu(), logp.cpu(), counts


def _const_model():
    """All weights zero except final_conv.bias: v = c exactly and (dv/dx)^T eps = 0."""
    from flocoder_amd.unet import Unet
    g = torch.Generator().manual_seed(11)
    m = Unet(dim=16, dim_mults=(1, 2, 4, 8), channels=4, n_classes=10).eval()
    sd = {k: torch.zeros_like(v) for k, v in m.state_dict().items()}
    c = torch.randn(4, generator=g)
    sd["final_conv.bias"] = c.clone()
    m.load_state_dict(sd, strict=True)
    x = torch.randn(2, 4, 16, 16, generator=g)
    x[1] *= 1e-3                                              # select_initial_step picks another first step: the samples step differently
    return m.to(DEV), c, x


def _scipy_counts(f, y0, t0=1.0, t1=0.0):
    from scipy.integrate import solve_ivp
    sol = solve_ivp(f, (t0, t1), y0, method="RK45", rtol=1e-5, atol=1e-5)
    acc = len(sol.t) - 1
    return [sol.nfev, acc, (sol.nfev - 2) // 6 - acc]


def test_controller_exact_on_a_constant_field_backwards():
    """v = c, g = 0: a must stay exactly 0.0, z = x - (t0 - t1) c, and (nfev, accepted, rejected) must EQUAL scipy's on the augmented
    system [x, a] solved from 1 to 0, in both modes (n = m + spg in the norms; the first device test of the controller running
    backwards).  invert_latents(method="rk45") is the same solve on x alone: scipy's counters on x alone."""
    from flocoder_amd import sampling as S
    m, c, x = _const_model()
    eps = torch.where(torch.randn(x.shape, generator=torch.Generator().manual_seed(5)) >= 0, 1.0, -1.0)
    cfull = c.view(4, 1, 1).expand(4, 16, 16).double().numpy().reshape(-1)
    exact = (x.double() - c.double().view(1, 4, 1, 1)).float()
    aug = lambda rows: (lambda t, y: np.concatenate([np.tile(cfull, rows), np.zeros(rows)]))
    y0 = lambda xs: np.concatenate([xs.double().numpy().reshape(-1), np.zeros(xs.shape[0])])

    ref_ps = [_scipy_counts(aug(1), y0(x[b:b + 1])) for b in range(2)]
    z, a, logp, counts = _solve(m, x, eps, None, True)
    assert counts.tolist() == ref_ps, (counts.tolist(), ref_ps)
    assert ref_ps[0] != ref_ps[1]
    assert bool((a == 0.0).all()) and not bool(torch.signbit(a).any())
    for b in range(2):
        assert rel_l2(z[b], exact[b]) < 1e-6
    D = x[0].numel()
    assert float((logp + 0.5 * z.double().flatten(1).pow(2).sum(1) + 0.5 * D * math.log(2 * math.pi)).abs().max()) <= 1e-12 * float(logp.abs().max())

    ref_c = _scipy_counts(aug(2), y0(x))
    z, a, _, counts = _solve(m, x, eps, None, False)
    assert counts.tolist() == [ref_c], (counts.tolist(), ref_c)
    assert bool((a == 0.0).all()) and rel_l2(z, exact) < 1e-6

    # a partial interval, and the inversion's counters against scipy on x alone
    z, a, _, counts = _solve(m, x, eps, None, False, t0=0.9, t1=0.25)
    assert counts.tolist() == [_scipy_counts(aug(2), y0(x), 0.9, 0.25)] and rel_l2(z, (x.double() - 0.65 * c.double().view(1, 4, 1, 1)).float()) < 1e-6
    plain = lambda rows: (lambda t, y: np.tile(cfull, rows))
    zi, nfe = S.invert_latents(m, x.to(DEV), method="rk45", per_sample=False)
    assert nfe == _scipy_counts(plain(2), x.double().numpy().reshape(-1))[0] and rel_l2(zi.cpu(), exact) < 1e-6
    zi, nfe = S.invert_latents(m, x.to(DEV), method="rk45", per_sample=True)
    assert nfe == max(_scipy_counts(plain(1), x[b].double().numpy().reshape(-1))[0] for b in range(2)) and rel_l2(zi.cpu(), exact) < 1e-6


@pytest.mark.parametrize("mode", ["ps", "coupled"])
@pytest.mark.parametrize("cid", list(rr.CASES))
def test_against_the_scipy_golden(cid, mode):
    g = load_golden("ll_rk45_scipy_oracle")
    sd, x, eps, cond = _case(cid)
    ref = {k: g[f"{cid}.{mode}.{k}"] for k in ("z", "a", "logp", "counts", "gsum")}
    assert (ref["counts"][:, 2] >= 1).all()                     # the fixture exercises the rejection path
    per_sample = mode == "ps"
    z, a, logp, counts = _solve(_model(sd), x, eps, cond, per_sample)
    assert torch.isfinite(z).all() and torch.isfinite(logp).all() and a.dtype == torch.float64
    zr = torch.from_numpy(ref["z"])
    en = eps.double().flatten(1).norm(dim=1)
    bound = G_TOL * en * torch.from_numpy(ref["gsum"]) + 2 * torch.from_numpy(np.abs(ref["a"] - g[f"{cid}.a_tight"]))
    ratio = (a - torch.from_numpy(ref["a"])).abs() / bound
    lb = bound + 0.5 * (z.double().flatten(1).pow(2).sum(1) - zr.double().flatten(1).pow(2).sum(1)).abs()
    lratio = (logp - torch.from_numpy(ref["logp"])).abs() / lb
    zerr = [rel_l2(z[b], zr[b]) for b in range(x.shape[0])]
    print(f"\n[{cid} {mode}] counters {counts.tolist()} (scipy {ref['counts'].tolist()}); z rel-L2 {zerr}; a_gpu {a.tolist()}, a_ref {ref['a'].tolist()}, "
          f"bound {bound.tolist()}, |a_gpu - a_ref| / bound {ratio.tolist()}; |logp_gpu - logp_ref| / bound {lratio.tolist()}")
    assert max(zerr) < TRAJ_TOL, zerr
    assert bool(((counts[:, 0] - torch.from_numpy(ref["counts"][:, 0])).abs() <= NFEV_SLACK).all()), (counts.tolist(), ref["counts"].tolist())
    assert bool((ratio <= 1).all()), ratio
    assert bool((lratio <= 1).all()), lratio
    # the public entry point is this call
    from flocoder_amd import sampling as S
    lp, zp, nfe = S.log_likelihood(_model(sd), x.to(DEV), cond=_dcond(cond), probe=eps.to(DEV), method="rk45", per_sample=per_sample)
    assert torch.equal(lp.cpu(), logp) and torch.equal(zp.cpu(), z) and nfe == int(counts[:, 0].max())


def test_repeat_is_bitwise_and_a_batch_of_one_is_the_coupled_solve():
    """Two calls give equal bits (logp, a, z, counters), in both modes.  A batch of one is the same solve_ivp problem in both modes, and
    while C*H*W <= 64 * 1024 the per-sample reduction partition is the coupled one: equal bits."""
    sd, x, eps, cond = _case("d16c10-class")
    model = _model(sd)
    for per_sample in (True, False):
        r1, r2 = _solve(model, x, eps, cond, per_sample), _solve(model, x, eps, cond, per_sample)
        assert all(torch.equal(p, q) for p, q in zip(r1, r2))
    one = {k: v[:1] for k, v in cond.items()}
    p, c = _solve(model, x[:1], eps[:1], one, True), _solve(model, x[:1], eps[:1], one, False)
    assert all(torch.equal(u, v) for u, v in zip(p, c))


def test_a_sample_does_not_depend_on_its_batchmates():
    """First: is one evaluation (training-form forward, data-gradient chain) of a row bit-equal in a batch of 1 and of 3?  If yes, the
    per-sample solve of that row must be bit-equal too (logp, z, counters).  If not, the two calls are two valid solves of one problem
    and are held to the golden gate's bounds against each other (the finding is in DESIGN.md section 4)."""
    cid = "d16c10-class"
    g = load_golden("ll_rk45_scipy_oracle")
    sd, x, eps, cond = _case(cid)
    model = _model(sd, train=True)
    gen = torch.Generator().manual_seed(91)
    x3 = torch.cat([x[:1], 2.0 * torch.randn(2, *x.shape[1:], generator=gen)])
    e3 = torch.cat([eps[:1], eps[1:2], -eps[:1]])
    c3 = torch.cat([cond["class_cond"][:1], torch.tensor([0, 9])])
    td = torch.full((3,), 0.37 * 999, device=DEV)
    xd, ed, cd = x3.to(DEV), e3.to(DEV), c3.to(DEV)
    v3 = model._forward_native(xd, td, cd, None, train=True)
    g3 = model.vjp_x(xd, td, cd, ed)
    v1 = model._forward_native(xd[:1].clone(), td[:1], cd[:1], None, train=True)
    g1 = model.vjp_x(xd[:1].clone(), td[:1], cd[:1], ed[:1].clone())
    torch.cuda.synchronize()
    rowwise = torch.equal(v3[:1], v1) and torch.equal(g3[:1], g1)
    print(f"\none evaluation of a row, batch of 1 against batch of 3: forward equal {torch.equal(v3[:1], v1)}, d(x) equal {torch.equal(g3[:1], g1)}")
    model = _model(sd)
    z1, a1, l1, n1 = _solve(model, x3[:1], e3[:1], {"class_cond": c3[:1]}, True)
    z3, a3, l3, n3 = _solve(model, x3, e3, {"class_cond": c3}, True)
    if rowwise:
        assert torch.equal(l3[:1], l1) and torch.equal(z3[:1], z1) and torch.equal(n3[:1], n1)
        return
    bound = G_TOL * float(e3[0].double().norm()) * float(g[f"{cid}.ps.gsum"][0]) + 2 * abs(float(g[f"{cid}.ps.a"][0] - g[f"{cid}.a_tight"][0]))
    lb = bound + 0.5 * abs(float(z3[0].double().pow(2).sum() - z1[0].double().pow(2).sum()))
    print(f"not row-wise bit-equal: |a| diff {float((a3[0] - a1[0]).abs())} (bound {bound}), z rel-L2 {rel_l2(z3[0], z1[0])}, nfev {n3[0].tolist()} / {n1[0].tolist()}")
    assert rel_l2(z3[0], z1[0]) < TRAJ_TOL and abs(int(n3[0, 0]) - int(n1[0, 0])) <= NFEV_SLACK
    assert float((a3[0] - a1[0]).abs()) <= bound and float((l3[0] - l1[0]).abs()) <= lb


@pytest.mark.timeout(600)
def test_an_adaptive_likelihood_call_leaks_nothing():
    """Sampler, RK4 likelihood and both RK45 sampler modes give, after an adaptive likelihood call, the bits they gave before it in the
    same process, and the sampler those of a fresh model; a FlowTrainer.step pair around a call is bit-equal to one without."""
    from flocoder_amd import _binding as B
    from flocoder_amd import sampling as S
    from flocoder_amd.train import FlowTrainer
    from oracle.synth import synth_input, synth_state_dict
    gd = load_golden("g10_train_step")
    sd = synth_state_dict(gd["shapes"], 10)
    cls = torch.from_numpy(gd["cls"]).to(DEV)[:4]
    xl = (0.2 * synth_input("llrk45.hyg.x", (4, 4, 16, 16), 1)).to(DEV)
    el = torch.where(synth_input("llrk45.hyg.e", (4, 4, 16, 16), 1) >= 0, 1.0, -1.0).to(DEV)
    src = synth_input("llrk45.hyg.src", (4, 4, 16, 16), 2).to(DEV)
    cond = {"class_cond": cls}
    kw = dict(method="rk45", rtol=1e-2, atol=1e-2)           # a short solve: hygiene does not depend on the tolerance

    def calls(m):
        out = [S.generate_latents_rk4(m, (4, 4, 16, 16), 4, cond, 3.0, source=src)[0],
               S.log_likelihood(m, xl, n_steps=3, cond=cond, probe=el)[0]]
        for ps in (False, True):
            lat, nfe = S.rk45_sampler(m, (4, 4, 16, 16), cond=cond, source=src, rtol=1e-2, atol=1e-2, cfg_strength=3.0, per_sample=ps)
            out += [lat, torch.tensor(nfe)]
        torch.cuda.synchronize()
        return [o.clone() for o in out]

    used, fresh = _model(sd), _model(sd)
    before = calls(used)
    for ps in (True, False):
        lp, _, _ = S.log_likelihood(used, xl, cond=cond, probe=el, per_sample=ps, **kw)
        assert torch.isfinite(lp).all() and B.lib().fc_unet_train_form(used._handle) == 0
    after = calls(used)
    assert all(torch.equal(p, q) for p, q in zip(before, after))
    assert torch.equal(after[0], calls(fresh)[0]) and used.launches_per_forward == fresh.launches_per_forward

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
                lp, _, _ = S.log_likelihood(m, xl, cond=cond, probe=el, **kw)
                assert m.training and torch.isfinite(lp).all()
        torch.cuda.synchronize()
        return out

    for (l0, g0, p0), (l1, g1, p1) in zip(run(False), run(True)):
        assert torch.equal(l0, l1) and torch.equal(g0, g1) and torch.equal(p0, p1)


def test_refusals_on_the_gpu():
    from flocoder_amd import sampling as S
    sd, x, eps, cond = _case("d16c10-class")
    model = _model(sd)
    xd, ed, cd = x.to(DEV), eps.to(DEV), _dcond(cond)
    with pytest.raises(ValueError, match="guidance"):
        S.log_likelihood(model, xd, cond=cd, method="rk45", cfg_strength=3.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.log_likelihood(model, x, cond=cond, method="rk45")
    with pytest.raises(RuntimeError):
        model.log_likelihood_rk45(x.clone(), eps)
    with pytest.raises(RuntimeError):
        S.invert_latents(model, x, cond=cond, method="rk45")
    for t0, t1 in ((0.5, 0.5), (0.2, 0.7), (1.5, 0.0), (1.0, -0.1)):
        with pytest.raises(ValueError, match="t1"):
            model.log_likelihood_rk45(xd.clone(), ed, t0, t1, class_ids=cd["class_cond"])
    with pytest.raises(ValueError, match="shape"):
        S.log_likelihood(model, xd, cond=cd, method="rk45", probe=torch.ones(2, 4, 16, 8, device=DEV))
    with pytest.raises(ValueError, match="probe"):
        model.log_likelihood_rk45(xd.clone(), ed[:1], class_ids=cd["class_cond"])
    with pytest.raises(ValueError, match="atol"):
        model.log_likelihood_rk45(xd.clone(), ed, atol=-1.0, class_ids=cd["class_cond"])
    from flocoder_amd import _binding as B
    assert B.lib().fc_unet_train_form(model._handle) == 0 and torch.equal(xd.cpu(), x)
