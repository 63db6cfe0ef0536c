"""Per-sample adaptive RK45 on the device (fc_unet_integrate_rk45_per_sample, Unet.integrate_rk45(per_sample=True),
generate_latents(method="rk45_per_sample"), sample_many) against its contract: every sample b is its own
scipy.integrate.solve_ivp(method="RK45", rtol = atol = 1e-5) problem over (1e-3, 1) around the CPU oracle U-Net on that sample alone
(tools/make_rk45_per_sample_golden.py wrote tests/golden/rk45_per_sample_scipy_oracle.npz from it).

Gates as in test_gpu_rk45.py, per sample: rel-L2 < 2e-4 on the latents and |nfev - scipy's| <= 12 (two attempts: an accept / reject
decision right at error_norm ~ 1 can fall the other way under the U-Net's ~1e-6 differences).  Two trajectories are less well
conditioned than that gate assumes: with the oracle alone, multiplying every evaluation by (1 + 1e-7 randn) moves the final latents of
d16_cfg0 sample 0 by 3.4e-5 and of d16_mixed sample 0 by 7.4e-5 (rel-L2; d16_cfg3 sample 0: 7.9e-7), so the device's ~1e-6 forward
differences move them by ~4e-4.  Those two cases are gated at TRAJ_TOL_ILL; what ties them to the validated batch-coupled path exactly
is test_batch_of_one_equals_the_coupled_solve.  The constant-field case has no U-Net rounding, so there the counters must EQUAL scipy's.
Within one call a sample's result must not depend on its batchmates at all."""
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, load_golden, rel_l2

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TRAJ_TOL, NFEV_SLACK = 2e-4, 12
TRAJ_TOL_ILL = {"d16_cfg0": 1e-3, "d16_mixed": 1e-3}
GOLDEN = "rk45_per_sample_scipy_oracle"


def _device_model(sd, **kw):
    from flocoder_amd.unet import Unet
    m = Unet(dim_mults=(1, 2, 4, 8), channels=4, **kw).eval()
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


def _model_kw(name):
    from tools.make_rk45_golden import CASES
    kw = CASES["d16_cfg0" if name == "d16_mixed" else name][0]
    return dict(dim=8, n_classes=0, mask_cond=True) if kw == "d8mask" else kw


def _case(name):
    from tools.make_rk45_per_sample_golden import per_sample_inputs
    sd, _, cond, cfg = per_sample_inputs(name)
    g = load_golden(GOLDEN)
    z0 = torch.from_numpy(g[f"{name}.source"])
    return _device_model(sd, **_model_kw(name)), z0, cond, cfg, torch.from_numpy(g[f"{name}.latents"]), g[f"{name}.counts"]


def _dcond(cond):
    return {k: (v.to(DEV) if v is not None else None) for k, v in cond.items()}


def _solve(model, z0, cond, cfg):
    """Unet.integrate_rk45(per_sample=True) as rk45_sampler drives it: (latents on the host, [B, 3] counters)."""
    from flocoder_amd.sampling import _mask_flags
    dcond = _dcond(cond)
    mask, ones = _mask_flags(dcond)
    x = z0.to(DEV).contiguous().clone()
    nfev, acc, rej = model.integrate_rk45(x, 1e-3, 1.0, rtol=1e-5, atol=1e-5, class_ids=dcond.get("class_cond"), cfg_strength=cfg,
                                          mask=mask, mask_is_ones=ones, per_sample=True)
    assert nfev.dtype == torch.int64 and nfev.shape == (z0.shape[0],)
    return x.cpu(), torch.stack([nfev, acc, rej], 1)


def _check_vs_oracle(lat, counts, ref, ref_counts, tol=TRAJ_TOL):
    for b in range(lat.shape[0]):
        err = rel_l2(lat[b], ref[b])
        assert err < tol and abs(int(counts[b, 0]) - int(ref_counts[b][0])) <= NFEV_SLACK, (b, err, counts.tolist(), ref_counts.tolist())


def test_controllers_exact_on_a_constant_field():
    """All weights zero except final_conv.bias: v = c exactly.  A source of unit scale and one scaled by 1e-3 make select_initial_step
    pick different first steps, so the two samples take different step sequences; each sample's (nfev, accepted, rejected) must EQUAL
    scipy's on that sample alone, and the result is z0 + (1 - 1e-3) c."""
    from scipy.integrate import solve_ivp
    from flocoder_amd.unet import Unet
    g = torch.Generator().manual_seed(11)
    m = Unet(dim=16, dim_mults=(1, 2, 4, 8), channels=4, n_classes=10).eval()
    sd = {k: torch.zeros_like(v) for k, v in m.state_dict().items()}
    c = torch.randn(4, generator=g)
    sd["final_conv.bias"] = c.clone()
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    z0 = torch.randn(2, 4, 16, 16, generator=g)
    z0[1] *= 1e-3
    cfull = c.view(4, 1, 1).expand(4, 16, 16).double().numpy().reshape(-1)
    ref = []
    for b in range(2):
        sol = solve_ivp(lambda t, y: cfull, (1e-3, 1), z0[b].numpy().reshape(-1), method="RK45", rtol=1e-5, atol=1e-5)
        acc = len(sol.t) - 1
        ref.append((sol.nfev, acc, (sol.nfev - 2) // 6 - acc))
    assert [r[0] for r in ref] == [20, 32]                   # scipy 1.15
    x = z0.to(DEV).contiguous().clone()
    nfev, accepted, rejected = m.integrate_rk45(x, 1e-3, 1.0, rtol=1e-5, atol=1e-5, per_sample=True)
    assert [tuple(int(v) for v in r) for r in zip(nfev, accepted, rejected)] == ref, (nfev, accepted, rejected, ref)
    exact = (z0.double() + (1 - 1e-3) * c.double().view(1, 4, 1, 1)).float()
    for b in range(2):
        assert rel_l2(x.cpu()[b], exact[b]) < 1e-6


@pytest.mark.parametrize("name", ["d16_cfg0", "d16_cfg3", "d8mask", "d32", "d16_mixed"])
def test_fixture_cases_vs_per_sample_scipy_oracle(name):
    """d16 without and with CFG, the dim-8 mask-conditioned model at 4x8x8 (the one-workgroup-per-sample plan, config 5), the headline
    shape, and samples of different scales whose step counts differ (each with rejections)."""
    model, z0, cond, cfg, ref, ref_counts = _case(name)
    if name == "d16_mixed":
        assert len(set(int(v) for v in ref_counts[:, 0])) == ref_counts.shape[0] and (ref_counts[:, 2] >= 1).all()
    lat, counts = _solve(model, z0, cond, cfg)
    _check_vs_oracle(lat, counts, ref, ref_counts, TRAJ_TOL_ILL.get(name, TRAJ_TOL))


@pytest.mark.parametrize("name", ["d16_cfg0", "d16_cfg3", "d8mask", "d32"])
def test_batch_of_one_equals_the_coupled_solve(name):
    """A batch of one is the same solve_ivp problem in both modes, and while C*H*W <= 64 * 1024 the per-sample reduction partition is the
    coupled one: sample 0 alone must give the coupled solve's latents and nfev bit for bit."""
    from flocoder_amd import sampling as S
    model, z0, cond, cfg, _, _ = _case(name)
    one = {k: (v[:1] if v is not None else None) for k, v in cond.items()}
    lat, counts = _solve(model, z0[:1], one, cfg)
    ref, nfe = S.generate_latents_rk45(model, (1,) + tuple(z0.shape[1:]), cond=_dcond(one), cfg_strength=cfg, source=z0[:1].to(DEV))
    assert torch.equal(lat, ref.cpu()) and int(counts[0, 0]) == nfe


@pytest.mark.parametrize("name", ["d16_mixed", "d16_cfg3"])
def test_a_sample_does_not_depend_on_its_batchmates(name):
    """Same batch size, sample 1's source and class id changed: sample 0's latents and counters are bit-identical."""
    model, z0, cond, cfg, _, _ = _case(name)
    lat, counts = _solve(model, z0, cond, cfg)
    z1 = z0.clone()
    z1[1] = 3.0 * torch.randn(z0.shape[1:], generator=torch.Generator().manual_seed(77))
    cond1 = dict(cond)
    cond1["class_cond"] = cond["class_cond"].clone()
    cond1["class_cond"][1] = 0
    lat1, counts1 = _solve(model, z1, cond1, cfg)
    assert not torch.equal(lat1[1], lat[1])
    assert torch.equal(lat1[0], lat[0]) and torch.equal(counts1[0], counts[0]), (counts.tolist(), counts1.tolist())


def test_a_batch_split_in_two_calls_matches_one_call():
    """What sharding across ranks does: a batch of 4 solved as two calls of 2 matches the single call (plans may differ with B)."""
    model, z0, cond, cfg, _, _ = _case("d16_cfg3")
    z4 = torch.cat([z0, 2.0 * z0.flip(0)])
    cond4 = {"class_cond": torch.tensor([5, 8, 1, 9])}
    whole, cw = _solve(model, z4, cond4, cfg)
    a, ca = _solve(model, z4[:2], {"class_cond": cond4["class_cond"][:2]}, cfg)
    b, cb = _solve(model, z4[2:], {"class_cond": cond4["class_cond"][2:]}, cfg)
    split, cs = torch.cat([a, b]), torch.cat([ca, cb])
    for i in range(4):
        assert rel_l2(split[i], whole[i]) < 1e-5, (i, rel_l2(split[i], whole[i]))
    assert (cs[:, 0] - cw[:, 0]).abs().max() <= NFEV_SLACK, (cs.tolist(), cw.tolist())


def test_sample_many_matches_one_at_a_time():
    """sample_many runs its replicas on the plan without cross-workgroup waits (equal to the default one to fp32 rounding), so the
    one-at-a-time calls use that plan as well."""
    from flocoder_amd import sampling as S
    model, z0, cond, cfg, _, _ = _case("d16_cfg3")
    shape = tuple(z0.shape)
    batches = [({"class_cond": cond["class_cond"].to(DEV)}, z0.to(DEV)),
               ({"class_cond": cond["class_cond"].flip(0).to(DEV)}, (0.5 * z0).to(DEV))]
    model.set_shared_device(True)
    try:
        single = [S.generate_latents(model, shape, method="rk45_per_sample", cond=c, cfg_strength=cfg, source=s)[0].cpu() for c, s in batches]
    finally:
        model.set_shared_device(None)
    many = S.sample_many(model, shape, batches, method="rk45_per_sample", cfg_strength=cfg, in_flight=2)
    assert len(many) == 2
    for a, b in zip(many, single):
        assert rel_l2(a.cpu(), b) < 1e-6


def test_repeat_is_bitwise_and_generate_latents_reports_max_nfev():
    from flocoder_amd import sampling as S
    model, z0, cond, cfg, _, _ = _case("d16_cfg3")
    a, ca = _solve(model, z0, cond, cfg)
    b, cb = _solve(model, z0, cond, cfg)            # replays the cached attempt graph
    assert torch.equal(a, b) and torch.equal(ca, cb)
    lat, nfe = S.generate_latents(model, tuple(z0.shape), method="rk45_per_sample", cond=_dcond(cond), cfg_strength=cfg, source=z0.to(DEV))
    assert torch.equal(lat.cpu(), a) and nfe == int(ca[:, 0].max())


def test_coupled_mode_unchanged_after_a_per_sample_solve():
    """The batch-coupled "rk45" shares its buffers and graph cache with the per-sample mode: after a per-sample solve on the same Unet it
    must give, bit for bit, what a fresh Unet gives."""
    from flocoder_amd import sampling as S
    model, z0, cond, cfg, _, _ = _case("d16_cfg0")
    fresh, _, _, _, _, _ = _case("d16_cfg0")
    ref, nref = S.generate_latents_rk45(fresh, tuple(z0.shape), cond=_dcond(cond), cfg_strength=cfg, source=z0.to(DEV))
    _solve(model, z0, cond, cfg)
    got, ngot = S.generate_latents_rk45(model, tuple(z0.shape), cond=_dcond(cond), cfg_strength=cfg, source=z0.to(DEV))
    assert torch.equal(got, ref) and ngot == nref


_CHILD = r"""
import json, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import torch
from test_gpu_rk45_per_sample import _case, _solve
from conftest import rel_l2
out = []
for name in ("d16_cfg0", "d16_mixed"):
    model, z0, cond, cfg, ref, counts = _case(name)
    lat, c = _solve(model, z0, cond, cfg)
    out.append(dict(case=name, rel_l2=[rel_l2(lat[b], ref[b]) for b in range(lat.shape[0])], nfev=c[:, 0].tolist(),
                    nfev_ref=[int(v) for v in counts[:, 0]], finite=bool(torch.isfinite(lat).all())))
print(json.dumps(dict(env=__import__("os").environ.get("AMD_DIRECT_DISPATCH"), calls=out)))
"""


@pytest.mark.skipif(os.environ.get("FLOCODER_AMD_IN_CHILD_SUITE") == "1", reason="already inside the child suite")
def test_two_calls_under_the_shipping_environment():
    """AMD_DIRECT_DISPATCH=0 (the mode the sampler ships with), a fresh process: two consecutive calls with different sources, class ids
    and batch sizes, each against the per-sample scipy oracle."""
    env = {k: v for k, v in os.environ.items() if k != "FLOCODER_AMD_KEEP_ENV"}
    env["AMD_DIRECT_DISPATCH"] = "0"
    env["FLOCODER_AMD_IN_CHILD_SUITE"] = "1"
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    recs = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert r.returncode == 0 and recs, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    rec = recs[-1]
    assert rec["env"] == "0"
    for c in rec["calls"]:
        assert c["finite"] and max(c["rel_l2"]) < TRAJ_TOL_ILL.get(c["case"], TRAJ_TOL), rec
        assert all(abs(a - b) <= NFEV_SLACK for a, b in zip(c["nfev"], c["nfev_ref"])), rec
