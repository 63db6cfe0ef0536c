"""Stochastic (SDE) sampling on the GPU (fc_ode_normal_field, fc_unet_integrate_sde) against the host form of the noise field
(flocoder_amd/noise.py) and the fp64 restatement over the oracle U-Net (tests/sde_ref.py).  Cases: tests/guided_ref.py CASES (the likelihood
test's models), sigma = 1.

Gates, none of them measured on the code under test:
  field          per value, from the documented operation sequence (ode.hip box_muller).  The uniforms are exact
                 fp32 numbers, 2 u is exact, so with u = 2^-24 the rounded quantities are: logf (documented 1 ulp <= 2u relative; -2 x is
                 exact; the square root at most halves it, counted whole here), the correctly rounded square root (1u), sincospif on an
                 exact argument (documented 1 ulp <= 2u of each result) and the product (1u): |z - z64| <= N u |z| with N = 6.  One wrong
                 bit in a uniform moves the angle by 2 pi 2^-23 = 7.5e-7 R, twice the bound of a typical value, and a wrong Philox word
                 moves everything: the integer stage cannot hide behind the bound.  The same sample id gives EQUAL bits in every batch.
  trajectories   per-sample relative L2 < TRAJ_TOL = 2e-4 against the restatement (tests/test_gpu_unet.py's gate), supplied noise
  batching       rows with the same sample id, start and class id in B = 2 and B = 8 on one reservation: rel-L2 < 1e-5, the tolerance
                 tests/test_gpu_rk45_per_sample.py uses for a batch split in two calls
With -s every case prints its figures.

Measured on the MI355X (worst sample per case; also in DESIGN.md section 4b):
  field                    at most 0.50 of the bound over 19 712 values (60 % of them equal the rounded fp64 value)
  trajectories             Euler-Maruyama / Heun: d16c10 class ids 1.2e-6 / 1.2e-6 (cfg 0), 2.4e-6 / 2.3e-6 (cfg 3); d16c10 unconditioned
                           1.8e-6 / 1.7e-6; d32c102 1.6e-6 / 1.2e-6; d8mask 1.5e-6 / 1.2e-6; sigma = 0 at most 1.7e-6; without graphs (child
                           process, d16c10 cfg 3) 2.4e-6 / 2.3e-6
  generated vs supplied    bit-equal, both schemes
  B = 2 against B = 8      rel-L2 0, both schemes"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sde_ref as sr
from conftest import ROOT, rel_l2
from oracle import flow_oracle as fo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRAJ_TOL = 2e-4
BATCH_TOL = 1e-5
U = 2.0 ** -24
N_FIELD = 6


def _model(sd):
    from flocoder_amd.unet import Unet
    m = fo.unet_meta(sd)
    model = Unet(dim=m["dim"], dim_mults=(1, 2, 4, 8), channels=4, n_classes=m["n_classes"], mask_cond=m["mask_cond"])
    model.load_state_dict(sd, strict=True)
    return model.to(DEV).eval()


def _dev(cond):
    return None if cond is None else {k: v.to(DEV) for k, v in cond.items()}


def _rel(a, b):
    a, b = a.double().cpu().flatten(1), b.double().cpu().flatten(1)
    return (a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-300)


def _sde(model, c, method, cfg=None, sigma=sr.SIGMA, noise="case", **kw):
    from flocoder_amd import sampling as S
    if isinstance(noise, str):
        noise = c["noise"].to(DEV)
    lat, nfe = S.generate_latents_sde(model, tuple(c["source"].shape), n_steps=c["n"], cond=_dev(c["cond"]),
                                      cfg_strength=c["cfg"] if cfg is None else cfg, source=c["source"].to(DEV), sigma=sigma, method=method,
                                      noise=noise, **kw)
    torch.cuda.synchronize()
    return lat, nfe


def _device_field(seed, draw, ids, shape):
    from flocoder_amd import sampling as S
    out = S.normal_field(seed, draw, torch.as_tensor(ids, dtype=torch.int64), shape, DEV)
    torch.cuda.synchronize()
    return out


def test_field_matches_the_host_form_within_the_derived_bound():
    from flocoder_amd import _binding as B
    from flocoder_amd import noise as N
    worst, n_equal, n_all = 0.0, 0, 0
    for seed, draw, ids, shape in ((0, 0, np.arange(4), (4, 4, 32, 32)), ((0xfeedbeef << 32) | 77, 63, np.array([2 ** 40 + 5, 3, -1]), (3, 4, 16, 16)),
                                   (1234, 2 ** 32 - 1, np.array([9]), (1, 4, 8, 8))):
        got = _device_field(seed, draw, ids, shape).cpu().double().flatten(1)
        ref = torch.from_numpy(N.normal_field(seed, draw, ids, got.shape[1]))
        err, bound = (got - ref).abs(), N_FIELD * U * ref.abs()
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        n_equal += int((got.float() == ref.float()).sum()); n_all += got.numel()
        assert bool((err <= bound).all()), (seed, draw, float((err / bound.clamp_min(1e-300)).max()))
        assert float(got.abs().max()) <= N.TAIL * (1 + N_FIELD * U)
    print(f"\nworst |z - z64| / bound: {worst:.3f}; {n_equal} of {n_all} values equal the rounded fp64 value")
    # NULL sample ids are 0 .. B-1
    a = torch.empty(2, 64, device=DEV)
    B.check(B.lib().fc_ode_normal_field(B.ptr(a), 5, 1, None, 2, 64, B.current_stream(a.device)))
    torch.cuda.synchronize()
    assert torch.equal(a, _device_field(5, 1, [0, 1], (2, 64)))
    for args in ((B.ptr(a) + 4, 5, 1, None, 2, 60), (B.ptr(a), 5, -1, None, 2, 64), (B.ptr(a), 5, 1, None, 2, 62), (B.ptr(a), 5, 1, None, 0, 64)):
        with pytest.raises(ValueError):
            B.check(B.lib().fc_ode_normal_field(*args, B.current_stream(a.device)))


def test_a_sample_id_gives_the_same_bits_in_every_batch():
    shape = (4, 16, 16)
    two = _device_field(21, 4, [3, 9], (2,) + shape)
    eight = _device_field(21, 4, [7, 7, 9, 1, 3, 0, 2 ** 35, 9], (8,) + shape)
    one = _device_field(21, 4, [9], (1,) + shape)
    assert torch.equal(two[0], eight[4]) and torch.equal(two[1], eight[2]) and torch.equal(two[1], eight[7]) and torch.equal(one[0], two[1])
    assert torch.equal(eight[0], eight[1]) and not torch.equal(eight[0], eight[3])
    for other in (_device_field(22, 4, [9], (1,) + shape), _device_field(21, 5, [9], (1,) + shape), _device_field(21, 4, [10], (1,) + shape)):
        assert not torch.equal(other, one)


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("method", sr.SCHEMES)
@pytest.mark.parametrize("cid", list(sr.CASES))
def test_trajectories_match_the_fp64_restatement(cid, method):
    """Supplied noise; without guidance and, where the case has one, at the case's cfg_strength; then sigma = 0 against the restatement's
    deterministic Euler / Heun step, equal for two seeds."""
    c = sr.case_inputs(cid)
    model = _model(c["sd"])
    k = 2 if method == "heun" else 1
    for cfg in sorted({0.0, c["cfg"]}):
        lat, nfe = _sde(model, c, method, cfg=cfg)
        ref = sr.case_ref(cid, method, cfg)
        r = _rel(lat, ref)
        print(f"\n[{cid} {method} cfg {cfg}] rel-L2 to the restatement {r.tolist()}")
        assert nfe == (c["n"] - 1) * k and torch.isfinite(lat).all()
        assert float(r.max()) < TRAJ_TOL, r
    d1, _ = _sde(model, c, method, sigma=0.0, noise=None, seed=1)
    d2, _ = _sde(model, c, method, sigma=0.0, noise=None, seed=2)
    det = sr.case_ref(cid, method, c["cfg"], sigma=0.0)
    r0 = _rel(d1, det)
    print(f"[{cid} {method}] sigma = 0 rel-L2 to the deterministic restatement {r0.tolist()}")
    assert torch.equal(d1, d2) and float(r0.max()) < TRAJ_TOL
    assert float(_rel(lat, det).min()) > 1e-2                       # and with sigma = 1 it is another trajectory


_CHILD = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import torch
import sde_ref as sr
import test_gpu_sde as T
cid = "d16c10-class-cfg3"
c = sr.case_inputs(cid)
m = T._model(c["sd"])
out = []
for method in sr.SCHEMES:
    lat, _ = T._sde(m, c, method)
    out.append(float(T._rel(lat, sr.case_ref(cid, method, c["cfg"])).max()))
g1, _ = T._sde(m, c, "heun", noise=None, seed=3)
g2, _ = T._sde(m, c, "heun", noise=None, seed=3)
print("RESULT", out[0], out[1], int(torch.equal(g1, g2)))
"""


@pytest.mark.timeout(900)
def test_direct_launches_without_graphs_in_a_child_process():
    """FLOCODER_AMD_NO_GRAPH set (read once per process, hence the child, under its own time limit): the trajectory gate for one case."""
    env = dict(os.environ)
    env["FLOCODER_AMD_NO_GRAPH"] = "1"
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=800, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")]
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    _, em, heun, same = lines[-1].split()
    print(f"\nno-graph child: rel-L2 to the restatement, Euler-Maruyama {em}, Heun {heun}; same seed equal {same}")
    assert float(em) < TRAJ_TOL and float(heun) < TRAJ_TOL and same == "1"


@pytest.mark.parametrize("method", sr.SCHEMES)
def test_generated_noise_is_the_field(method):
    """A generated-noise run against a supplied-noise run fed fc_ode_normal_field's output for the same seed and ids; twice the same seed."""
    cid = "d16c10-class-cfg3"
    c = sr.case_inputs(cid)
    model = _model(c["sd"])
    shape = tuple(c["source"].shape)
    seed, ids = (3 << 32) | 17, torch.tensor([40, 2, 2 ** 33 + 1])
    xi = torch.stack([_device_field(seed, i, ids, shape) for i in range(c["n"] - 1)])
    sup, _ = _sde(model, c, method, noise=xi)
    gen, _ = _sde(model, c, method, noise=None, seed=seed, sample_ids=ids.to(DEV))
    again, _ = _sde(model, c, method, noise=None, seed=seed, sample_ids=ids.to(DEV))
    r = _rel(gen, sup)
    print(f"\n[{method}] generated vs supplied rel-L2 {r.tolist()}, equal bits: {torch.equal(gen, sup)}")
    assert float(r.max()) < TRAJ_TOL and torch.equal(gen, again)
    other, _ = _sde(model, c, method, noise=None, seed=seed, sample_ids=torch.tensor([41, 2, 2 ** 33 + 1]).to(DEV))
    assert not torch.equal(other[0], gen[0]) and torch.equal(other[1:], gen[1:])     # only row 0's id moved


@pytest.mark.timeout(900)
@pytest.mark.parametrize("method", sr.SCHEMES)
def test_a_captured_graph_keeps_nothing_of_a_call(method):
    """Seed A, B, A; noise tensor 1, 2, 1; sigma 1, 0.5, 1 -- in one process on one handle: results 1 and 3 are equal, 2 differs.  Then the
    deterministic samplers on the same handle give a fresh model's bits."""
    from flocoder_amd import sampling as S
    cid = "d16c10-class-cfg3"
    c = sr.case_inputs(cid)
    used, fresh = _model(c["sd"]), _model(c["sd"])
    shape, cond, src = tuple(c["source"].shape), _dev(c["cond"]), c["source"].to(DEV)
    n1 = c["noise"].to(DEV)
    n2 = torch.randn(n1.shape, generator=torch.Generator().manual_seed(99)).to(DEV)
    for runs in ([dict(noise=None, seed=s) for s in (11, 12, 11)], [dict(noise=n) for n in (n1, n2, n1.clone())],
                 [dict(sigma=s) for s in (1.0, 0.5, 1.0)], [dict(noise=None, seed=5, sigma=s) for s in (1.0, 0.5, 1.0)]):
        a, b, a2 = (_sde(used, c, method, **kw)[0] for kw in runs)
        assert torch.equal(a, a2) and float(_rel(b, a).min()) > 1e-3, runs
    for m in (used, fresh):
        m.out = (S.generate_latents_rk4(m, shape, c["n"], cond, c["cfg"], source=src)[0], S.euler_sampler(m, shape, 8, cond=cond, source=src)[0],
                 S.euler_sampler(m, shape, 8, cond=cond, source=src, cfg_strength=c["cfg"])[0])
    torch.cuda.synchronize()
    for x, y in zip(used.out, fresh.out):
        assert torch.equal(x, y)
    assert used.launches_per_forward == fresh.launches_per_forward


@pytest.mark.parametrize("method", sr.SCHEMES)
def test_a_sample_does_not_depend_on_its_batch(method):
    """Rows with the same sample id, start and class id in a batch of 8 and a batch of 2 on the same reservation."""
    from flocoder_amd import sampling as S
    from oracle.synth import synth_input
    c = sr.case_inputs("d16c10-nocond")
    model = _model(c["sd"])
    model.reserve(8, 16, 16)
    src = synth_input("sde.batch.src", (8, 4, 16, 16), 3).to(DEV)
    ids = torch.arange(100, 108, dtype=torch.int64, device=DEV)
    kw = dict(n_steps=c["n"], cfg_strength=0.0, sigma=1.0, method=method, seed=77)
    big, _ = S.generate_latents_sde(model, (8, 4, 16, 16), source=src, sample_ids=ids, **kw)
    pick = torch.tensor([6, 3], device=DEV)
    small, _ = S.generate_latents_sde(model, (2, 4, 16, 16), source=src[pick].contiguous(), sample_ids=ids[pick].contiguous(), **kw)
    default, _ = S.generate_latents_sde(model, (2, 4, 16, 16), source=src[pick].contiguous(), **kw)         # ids 0, 1: other noise
    torch.cuda.synchronize()
    errs = [rel_l2(small[i], big[int(pick[i])]) for i in range(2)]
    print(f"\n[{method}] B = 2 against B = 8, same ids: rel-L2 {errs}")
    assert max(errs) < BATCH_TOL, errs
    assert min(rel_l2(default[i], small[i]) for i in range(2)) > 1e-2


def test_argument_errors():
    c = sr.case_inputs("d16c10-nocond")
    model = _model(c["sd"])
    x = c["source"].to(DEV).clone()
    ts = torch.tensor([0.0, 0.3, 0.7, 1.0])
    ok = dict(sigma=1.0, method="heun")
    with pytest.raises(ValueError, match="contiguous"):
        model.integrate_sde(x.permute(0, 1, 3, 2), ts, **ok)
    with pytest.raises(ValueError, match="contiguous"):
        model.integrate_sde(x.double(), ts, **ok)
    with pytest.raises(ValueError, match="aligned"):
        model.integrate_sde(torch.empty(x.numel() + 1, device=DEV)[1:].view(x.shape), ts, **ok)
    for bad in (torch.tensor([0.5]), torch.tensor([0.0, 0.6, 0.5, 1.0]), torch.tensor([-0.1, 0.5]), torch.tensor([0.5, 1.1])):
        with pytest.raises(ValueError, match="grid"):
            model.integrate_sde(x.clone(), bad, **ok)
    with pytest.raises(ValueError, match="sigma"):
        model.integrate_sde(x.clone(), ts, sigma=-0.5, method="heun")
    with pytest.raises(ValueError, match="method"):
        model.integrate_sde(x.clone(), ts, sigma=1.0, method="rk4")
    with pytest.raises(ValueError, match="noise"):
        model.integrate_sde(x.clone(), ts, noise=torch.zeros((4,) + tuple(x.shape), device=DEV), **ok)
    with pytest.raises(ValueError, match="noise"):
        model.integrate_sde(x.clone(), ts, noise=torch.zeros((3,) + tuple(x.shape)), **ok)                      # on the CPU
    with pytest.raises(ValueError, match="sample_ids"):
        model.integrate_sde(x.clone(), ts, sample_ids=torch.zeros(x.shape[0], dtype=torch.int32, device=DEV), **ok)
    with pytest.raises(ValueError, match="sample_ids"):
        model.integrate_sde(x.clone(), ts, sample_ids=torch.zeros(x.shape[0] + 1, dtype=torch.int64, device=DEV), **ok)
    out = model.integrate_sde(x.clone(), ts, **ok)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and not torch.equal(out, x)
