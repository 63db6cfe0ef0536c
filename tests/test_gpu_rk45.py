"""Adaptive RK45 on the device (fc_unet_integrate_rk45, Unet.integrate_rk45, sampling.rk45_sampler / generate_latents_rk45) against the
legacy sampler it mirrors: scipy.integrate.solve_ivp(method="RK45", rtol = atol = 1e-5) over (1e-3, 1) around the CPU oracle U-Net
(legacy/train_sd_flowers.py:78-107; tools/make_rk45_golden.py wrote tests/golden/rk45_scipy_oracle.npz from it).

Gates: the trajectory gate TRAJ_TOL on the latents, and |nfev - scipy's| <= 12 (two attempts: an accept / reject decision right at
error_norm ~ 1 can fall the other way under the U-Net's ~1e-6 differences).  The constant-field case has no U-Net rounding at all, so
there the counters must EQUAL scipy's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, rel_l2

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TRAJ_TOL, NFEV_SLACK = 2e-4, 12


def _device_model(sd, **kw):
    from flocoder_amd.unet import Unet
    m = Unet(dim_mults=(1, 2, 4, 8), channels=4, **kw).eval()
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


def _case(name):
    from tools.make_rk45_golden import CASES, case_inputs
    sd, _, cond, cfg = case_inputs(name)
    g = load_golden("rk45_scipy_oracle")
    kw = CASES[name][0]
    kw = dict(dim=8, n_classes=0, mask_cond=True) if kw == "d8mask" else kw
    z0 = torch.from_numpy(g[f"{name}.source"])
    return _device_model(sd, **kw), z0, cond, cfg, torch.from_numpy(g[f"{name}.latents"]), [int(v) for v in g[f"{name}.counts"]]


def _run(model, z0, cond, cfg):
    from flocoder_amd import sampling as S
    dcond = {k: (v.to(DEV) if v is not None else None) for k, v in cond.items()}
    lat, nfe = S.generate_latents_rk45(model, tuple(z0.shape), cond=dcond, cfg_strength=cfg, source=z0.to(DEV))
    return lat, nfe


def test_controller_exact_on_a_constant_field():
    """All weights zero except final_conv.bias: the forward returns exactly the bias, v = c.  scipy's nfev, accepted and attempts must be
    EQUAL (initial-step rule, growth clamp at MAX_FACTOR, t_bound clamp, termination), and the result z0 + (1 - 1e-3) c."""
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
    cfull = c.view(1, 4, 1, 1).expand_as(z0).double().numpy().reshape(-1)
    sol = solve_ivp(lambda t, y: cfull, (1e-3, 1), z0.numpy().reshape(-1), method="RK45", rtol=1e-5, atol=1e-5)
    acc = len(sol.t) - 1
    x = z0.to(DEV).contiguous().clone()
    nfev, accepted, rejected = m.integrate_rk45(x, 1e-3, 1.0, rtol=1e-5, atol=1e-5)
    assert (nfev, accepted, accepted + rejected) == (sol.nfev, acc, (sol.nfev - 2) // 6), (nfev, accepted, rejected, sol.nfev, acc)
    assert sol.nfev == 20 and acc == 3                       # t = 0.001, 0.0446, 0.4802, 1 (scipy 1.15)
    ref = (z0.double() + (1 - 1e-3) * c.double().view(1, 4, 1, 1)).float()
    assert rel_l2(x.cpu(), ref) < 1e-6
    assert rel_l2(x.cpu(), torch.from_numpy(sol.y[:, -1]).reshape(z0.shape)) < 1e-6


@pytest.mark.parametrize("name,scipy_rejects", [("d16_cfg0", 3), ("d16_cfg3", 4)])
def test_d16_vs_scipy_oracle(name, scipy_rejects):
    model, z0, cond, cfg, ref, (nfev_ref, _, rej_ref) = _case(name)
    assert rej_ref == scipy_rejects          # the fixture exercises the rejection path
    lat, nfe = _run(model, z0, cond, cfg)
    err = rel_l2(lat.cpu(), ref)
    assert err < TRAJ_TOL and abs(nfe - nfev_ref) <= NFEV_SLACK, (err, nfe, nfev_ref)


def test_per_sample_plan_with_mask_vs_scipy_oracle():
    """The dim-8 mask-conditioned model at 4x8x8 runs the one-workgroup-per-sample plan (config 5): its forwards take their time from the
    per-forward time row as well."""
    model, z0, cond, cfg, ref, (nfev_ref, _, _) = _case("d8mask")
    lat, nfe = _run(model, z0, cond, cfg)
    err = rel_l2(lat.cpu(), ref)
    assert err < TRAJ_TOL and abs(nfe - nfev_ref) <= NFEV_SLACK, (err, nfe, nfev_ref)


def test_headline_shape_vs_scipy_oracle():
    model, z0, cond, cfg, ref, (nfev_ref, _, rej_ref) = _case("d32")
    assert rej_ref >= 1
    lat, nfe = _run(model, z0, cond, cfg)
    err = rel_l2(lat.cpu(), ref)
    assert err < TRAJ_TOL and abs(nfe - nfev_ref) <= NFEV_SLACK, (err, nfe, nfev_ref)


def test_repeat_is_bitwise_and_sampler_decodes():
    from flocoder_amd import sampling as S
    model, z0, cond, cfg, _, _ = _case("d16_cfg0")
    a, na = _run(model, z0, cond, cfg)
    b, nb = _run(model, z0, cond, cfg)             # replays the cached attempt graph
    assert torch.equal(a, b) and na == nb

    class Codec(torch.nn.Module):
        def decode(self, z):
            return torch.nn.functional.interpolate(z[:, :3], scale_factor=2)

    lat, dec, nfe = S.sampler(model, Codec(), method="rk45", batch_size=2, latent_shape=(4, 16, 16), cond={"class_cond": cond["class_cond"].to(DEV)},
                              cfg_strength=0.0, source=z0.to(DEV), device=DEV)
    assert torch.equal(lat, a) and nfe == na and dec.shape == (2, 3, 32, 32) and torch.isfinite(dec).all()


_CHILD = r"""
import json, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import torch
from test_gpu_rk45 import _case, _run
from conftest import rel_l2
out = []
for name in ("d16_cfg0", "d16_other"):
    model, z0, cond, cfg, ref, counts = _case(name)
    lat, nfe = _run(model, z0, cond, cfg)
    out.append(dict(case=name, rel_l2=rel_l2(lat.cpu(), ref), nfe=nfe, nfev_ref=counts[0], finite=bool(torch.isfinite(lat).all())))
print(json.dumps(dict(env=__import__("os").environ.get("AMD_DIRECT_DISPATCH"), calls=out)))
"""


@pytest.mark.skipif(os.environ.get("FLOCODER_AMD_IN_CHILD_SUITE") == "1", reason="already inside the child suite")
def test_two_calls_under_the_shipping_environment():
    """AMD_DIRECT_DISPATCH=0 (the mode the sampler ships with), a fresh process: two consecutive calls with different sources and class ids,
    each against scipy + oracle.  Under this dispatch mode a graph replay has overtaken queued copies before (tests/test_gpu_shipping_env.py)."""
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
        assert c["finite"] and c["rel_l2"] < TRAJ_TOL and abs(c["nfe"] - c["nfev_ref"]) <= NFEV_SLACK, rec
