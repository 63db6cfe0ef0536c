"""Dense output of the adaptive RK45 on the device (fc_unet_integrate_rk45_dense, Unet.integrate_rk45(t_eval=...),
sampling.rk45_sampler / generate_latents_rk45(t_eval=...)) against its contract, solve_ivp's ``t_eval``: the solver steps exactly as it
would have, and every accepted step evaluates its quartic interpolant (scipy's RkDenseOutput) at the requested times inside it -- in
per-sample mode each sample's own steps.  tools/make_rk45_dense_golden.py wrote tests/golden/rk45_dense_scipy_oracle.npz from
solve_ivp(method="RK45", rtol = atol = 1e-5, t_eval=...) over (1e-3, 1) around the CPU oracle U-Net.

Gates are those of test_gpu_rk45.py / test_gpu_rk45_per_sample.py, applied to every frame: TRAJ_TOL on a trajectory (TRAJ_TOL_ILL for the
ill-conditioned d16_mixed), |nfev - scipy's| <= 12, 1e-6 and EQUAL counters on the constant field.  The bit equalities need no oracle:
they say that dense output reads the solve and never changes it, and that a replayed attempt graph serves whatever request the call
brought."""
import functools
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
TRAJ_TOL_ILL = {"d16_mixed": 1e-3}
SPLIT_TOL = 1e-5                   # test_a_batch_split_in_two_calls_matches_one_call's gate: plans may differ with the batch size
GOLDEN = "rk45_dense_scipy_oracle"
TE = [1e-3, 0.05, 0.25, 0.5, 0.75, 0.9, 1.0]
TE_CONST = [1e-3, 0.02, 0.1, 0.3, 0.4802, 0.75, 1.0]      # the constant field takes three steps (boundaries near 0.04 and 0.46): one step
                                                          # serves several values, one value lies just behind a boundary


def _model_kw(name):
    from tools.make_rk45_golden import CASES
    kw = CASES["d16_cfg0" if name == "d16_mixed" else name][0]
    return dict(dim=8, n_classes=0, mask_cond=True) if kw == "d8mask" else kw


def _fresh_model(name):
    from flocoder_amd.unet import Unet
    from tools.make_rk45_per_sample_golden import per_sample_inputs
    sd = per_sample_inputs(name)[0]
    m = Unet(dim_mults=(1, 2, 4, 8), channels=4, **_model_kw(name)).eval()
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def _model(name):
    return _fresh_model(name)


def _inputs(name):
    """(source, cond, cfg) of a case; the shared cases have the same inputs in both modes."""
    from tools.make_rk45_per_sample_golden import per_sample_inputs
    _, z0, cond, cfg = per_sample_inputs(name)
    return z0, cond, cfg


def _dcond(cond):
    return {k: (v.to(DEV) if v is not None else None) for k, v in cond.items()}


def _solve(model, z0, cond, cfg, per_sample, t_eval=None, t0=1e-3, t1=1.0):
    """Unet.integrate_rk45 as rk45_sampler drives it: (latents, counters [G, 3], frames or None), on the host."""
    from flocoder_amd.sampling import _mask_flags
    dcond = _dcond(cond) if cond else {}
    mask, ones = _mask_flags(dcond)
    x = z0.to(DEV).contiguous().clone()
    out = model.integrate_rk45(x, t0, t1, rtol=1e-5, atol=1e-5, class_ids=dcond.get("class_cond"), cfg_strength=cfg, mask=mask,
                               mask_is_ones=ones, per_sample=per_sample, t_eval=t_eval)
    assert len(out) == (3 if t_eval is None else 4)
    counts = torch.stack([torch.as_tensor(v, dtype=torch.int64).reshape(-1) for v in out[:3]], 1)
    frames = None
    if t_eval is not None:
        frames = out[3]
        assert frames.dtype == torch.float32 and frames.device == x.device and frames.shape == (len(t_eval),) + tuple(z0.shape)
        frames = frames.cpu()
    return x.cpu(), counts, frames


def _constant_model():
    """All weights zero except final_conv.bias: the forward returns exactly the bias, v = c."""
    from flocoder_amd.unet import Unet
    g = torch.Generator().manual_seed(11)
    m = Unet(dim=16, dim_mults=(1, 2, 4, 8), channels=4, n_classes=10).eval()
    sd = {k: torch.zeros_like(v) for k, v in m.state_dict().items()}
    c = torch.randn(4, generator=g)
    sd["final_conv.bias"] = c.clone()
    m.load_state_dict(sd, strict=True)
    z0 = torch.randn(2, 4, 16, 16, generator=g)
    return m.to(DEV), c, z0


@pytest.mark.parametrize("backwards", [False, True])
@pytest.mark.parametrize("per_sample", [False, True])
def test_constant_field_frames_and_counters(per_sample, backwards):
    """No U-Net rounding at all: every frame is float32(z0 + (te - t0) c) within the constant-field gate of
    test_controller_exact_on_a_constant_field (1e-6 rel-L2; scipy's own fp32 frames are there to 4e-8), the counters EQUAL those of scipy's
    solve with the same t_eval -- which are those without it -- and integrating backwards serves decreasing times."""
    from scipy.integrate import solve_ivp
    m, c, z0 = _constant_model()
    if per_sample:
        z0[1] *= 1e-3                                       # another first step, so the two samples take different step sequences
    t0, t1 = (1.0, 1e-3) if backwards else (1e-3, 1.0)
    te = TE_CONST[::-1] if backwards else TE_CONST
    ref_counts = []
    for rows in ([slice(0, 1), slice(1, 2)] if per_sample else [slice(0, 2)]):
        y0 = z0[rows]
        cfull = c.view(1, 4, 1, 1).expand_as(y0).double().numpy().reshape(-1)
        steps = []
        sol = solve_ivp(lambda t, y: cfull, (t0, t1), y0.numpy().reshape(-1), method="RK45", rtol=1e-5, atol=1e-5, t_eval=te,
                        events=lambda t, y: steps.append(t) or 1.0)
        acc = len(steps) - 1
        ref_counts.append([sol.nfev, acc, (sol.nfev - 2) // 6 - acc])
    if not backwards:
        assert [r[0] for r in ref_counts] == ([20, 32] if per_sample else [20])                     # scipy 1.15
    lat, counts, frames = _solve(m, z0, None, 0.0, per_sample, te, t0, t1)
    print("constant field", dict(per_sample=per_sample, backwards=backwards), counts.tolist(), ref_counts)
    assert counts.tolist() == ref_counts
    exact = (z0.double().unsqueeze(0) + (torch.tensor(te).view(-1, 1, 1, 1, 1) - t0) * c.double().view(1, 1, 4, 1, 1)).float()
    errs = [[rel_l2(frames[j, b], exact[j, b]) for b in range(2)] for j in range(len(te))]
    print("constant field frame errors", errs)
    assert max(max(e) for e in errs) < 1e-6, errs
    assert torch.equal(frames[0], z0)                       # te == t0: x = 0, the source
    lat0, counts0, _ = _solve(m, z0, None, 0.0, per_sample, None, t0, t1)
    assert torch.equal(lat, lat0) and torch.equal(counts, counts0)


@pytest.mark.parametrize("mode,name", [("coupled", "d16_cfg3"), ("coupled", "d8mask"), ("coupled", "d32"),
                                       ("per_sample", "d16_mixed"), ("per_sample", "d8mask")])
def test_fixture_frames_vs_scipy_oracle(mode, name):
    """Guidance (d16_cfg3), mask conditioning on the one-workgroup-per-sample plan of config 5 (d8mask), the headline shape (d32), and
    samples whose step sequences differ (d16_mixed): every frame under the trajectory gate of its case, per sample in per-sample mode."""
    g = load_golden(GOLDEN)
    key = f"{mode}.{name}"
    z0, cond, cfg = _inputs(name)
    assert np.array_equal(z0.numpy(), g[f"{key}.source"]) and g[f"{key}.t_eval"].tolist() == TE
    ref_frames, ref_lat = torch.from_numpy(g[f"{key}.frames"]), torch.from_numpy(g[f"{key}.latents"])
    ref_counts = torch.from_numpy(g[f"{key}.counts"]).reshape(-1, 3)
    per_sample = mode == "per_sample"
    lat, counts, frames = _solve(_model(name), z0, cond, cfg, per_sample, TE)
    rows = [slice(b, b + 1) for b in range(z0.shape[0])] if per_sample else [slice(None)]
    errs = [[rel_l2(frames[j, r], ref_frames[j, r]) for j in range(len(TE))] for r in rows]
    final = [rel_l2(lat[r], ref_lat[r]) for r in rows]
    print(key, "frame rel-L2 per controller:", errs, "final:", final, "nfev:", counts[:, 0].tolist(), "scipy:", ref_counts[:, 0].tolist())
    tol = TRAJ_TOL_ILL.get(name, TRAJ_TOL)
    assert max(max(e) for e in errs) < tol and max(final) < tol, (errs, final)
    assert (counts[:, 0] - ref_counts[:, 0]).abs().max() <= NFEV_SLACK, (counts.tolist(), ref_counts.tolist())
    assert torch.equal(frames[0], z0)


@pytest.mark.parametrize("per_sample", [False, True])
def test_t_eval_does_not_change_the_solve_and_repeats_bitwise(per_sample):
    """(a) latents and counters with t_eval == without, on one handle, in either order; (b) the frame at t0 is the source; (c) a repeat
    gives equal frames; (f) a list, a numpy array and a torch tensor of the same times give equal frames."""
    z0, cond, cfg = _inputs("d16_cfg3")
    model = _fresh_model("d16_cfg3")
    lat_d, counts_d, frames = _solve(model, z0, cond, cfg, per_sample, TE)                        # dense first ...
    lat_p, counts_p, _ = _solve(model, z0, cond, cfg, per_sample)
    assert torch.equal(lat_d, lat_p) and torch.equal(counts_d, counts_p)
    other = _fresh_model("d16_cfg3")
    lat_p2, counts_p2, _ = _solve(other, z0, cond, cfg, per_sample)                                # ... and plain first
    lat_d2, counts_d2, frames2 = _solve(other, z0, cond, cfg, per_sample, TE)
    assert torch.equal(lat_d2, lat_p2) and torch.equal(counts_d2, counts_p2) and torch.equal(lat_d2, lat_d)
    assert torch.equal(frames[0], z0)
    assert torch.equal(frames2, frames)
    assert rel_l2(frames[-1], lat_d) < 1e-6                  # the interpolant at x = 1 against y_new: equal to rounding, not in bits
    for te in (np.asarray(TE), torch.tensor(TE, dtype=torch.float64), torch.tensor(TE, dtype=torch.float64, device=DEV)):
        assert torch.equal(_solve(model, z0, cond, cfg, per_sample, te)[2], frames)


@pytest.mark.parametrize("name", ["d16_mixed", "d16_cfg3"])
def test_a_samples_frames_do_not_depend_on_its_batchmates(name):
    """(d) Same batch size, sample 1's source and class id changed: sample 0's frames, latents and counters are bit-identical."""
    z0, cond, cfg = _inputs(name)
    model = _model(name)
    lat, counts, frames = _solve(model, z0, cond, cfg, True, TE)
    z1 = z0.clone()
    z1[1] = 3.0 * torch.randn(z0.shape[1:], generator=torch.Generator().manual_seed(77))
    cond1 = dict(cond)
    cond1["class_cond"] = cond["class_cond"].clone()
    cond1["class_cond"][1] = 0
    lat1, counts1, frames1 = _solve(model, z1, cond1, cfg, True, TE)
    assert not torch.equal(frames1[:, 1], frames[:, 1])
    assert torch.equal(frames1[:, 0], frames[:, 0]) and torch.equal(lat1[0], lat[0]) and torch.equal(counts1[0], counts[0])


def test_frames_of_a_batch_split_in_two_calls():
    """(d) What sharding across ranks does: a batch of 4 solved as two calls of 2.  The plan may differ with the batch size, so the
    forwards -- and with them the final latents -- agree to rounding only (SPLIT_TOL, the gate of
    test_a_batch_split_in_two_calls_matches_one_call); the frames are held to that gate too, and where a sample's final latents and
    counters came out in equal bits its frames must be in equal bits as well: they are read off the same steps."""
    z0, _, cfg = _inputs("d16_cfg3")
    model = _model("d16_cfg3")
    z4 = torch.cat([z0, 2.0 * z0.flip(0)])
    ids = torch.tensor([5, 8, 1, 9])
    whole, cw, fw = _solve(model, z4, {"class_cond": ids}, cfg, True, TE)
    a, ca, fa = _solve(model, z4[:2], {"class_cond": ids[:2]}, cfg, True, TE)
    b, cb, fb = _solve(model, z4[2:], {"class_cond": ids[2:]}, cfg, True, TE)
    split, cs, fs = torch.cat([a, b]), torch.cat([ca, cb]), torch.cat([fa, fb], dim=1)
    errs = [[rel_l2(fs[j, i], fw[j, i]) for j in range(len(TE))] for i in range(4)]
    same = [bool(torch.equal(split[i], whole[i]) and torch.equal(cs[i], cw[i])) for i in range(4)]
    print("split: frame rel-L2", errs, "final latents and counters bit-equal:", same)
    assert max(max(e) for e in errs) < SPLIT_TOL, errs
    for i in range(4):
        if same[i]:
            assert torch.equal(fs[:, i], fw[:, i]), i


@pytest.mark.parametrize("name", ["d16_cfg3", "d8mask"])
def test_batch_of_one_per_sample_frames_equal_coupled_frames(name):
    """(e) A batch of one is the same solve_ivp problem in both modes (and the reduction partitions coincide)."""
    z0, cond, cfg = _inputs(name)
    one = {k: (v[:1] if v is not None else None) for k, v in cond.items()}
    model = _model(name)
    lat_p, counts_p, frames_p = _solve(model, z0[:1], one, cfg, True, TE)
    lat_c, counts_c, frames_c = _solve(model, z0[:1], one, cfg, False, TE)
    assert torch.equal(frames_p, frames_c) and torch.equal(lat_p, lat_c) and torch.equal(counts_p, counts_c)


@pytest.mark.parametrize("per_sample", [False, True])
def test_a_replayed_graph_serves_another_request(per_sample):
    """(g) A second call with other times of the same count and another frames tensor replays the cached attempt graph: times, count and
    destination live in device memory of the handle, so it must give what a fresh handle gives.  Then a longer and a shorter request."""
    z0, cond, cfg = _inputs("d16_cfg3")
    model = _fresh_model("d16_cfg3")
    te2 = [0.01, 0.1, 0.2, 0.4, 0.6, 0.8, 0.999]
    x = z0.to(DEV).contiguous().clone()
    first = model.integrate_rk45(x, 1e-3, 1.0, rtol=1e-5, atol=1e-5, class_ids=cond["class_cond"].to(DEV), cfg_strength=cfg,
                                 per_sample=per_sample, t_eval=TE)[3]                              # kept alive: the next frames tensor is another
    _, _, got = _solve(model, z0, cond, cfg, per_sample, te2)
    fresh = _fresh_model("d16_cfg3")
    _, _, ref = _solve(fresh, z0, cond, cfg, per_sample, te2)
    assert torch.equal(got, ref)
    assert torch.equal(first.cpu(), _solve(fresh, z0, cond, cfg, per_sample, TE)[2])               # and the first call's frames were not touched
    long = np.linspace(1e-3, 1.0, 33)
    _, _, f_long = _solve(model, z0, cond, cfg, per_sample, long)
    assert torch.equal(f_long[0], z0) and torch.equal(f_long[16], _solve(model, z0, cond, cfg, per_sample, [long[16]])[2][0])
    assert _solve(model, z0, cond, cfg, per_sample, [])[2].shape == (0,) + tuple(z0.shape)


@pytest.mark.parametrize("dense_first", [True, False])
def test_the_two_graph_shapes_do_not_leak_into_each_other(dense_first):
    """A call without t_eval after a call with it, and the reverse, each equal to the same call on a fresh model."""
    from flocoder_amd import sampling as S
    z0, cond, cfg = _inputs("d16_cfg3")
    shape, dcond, src = tuple(z0.shape), _dcond(cond), z0.to(DEV)
    model, fresh = _fresh_model("d16_cfg3"), _fresh_model("d16_cfg3")
    if dense_first:
        S.generate_latents_rk45(model, shape, cond=dcond, cfg_strength=cfg, source=src, t_eval=TE)
        got, ngot = S.generate_latents_rk45(model, shape, cond=dcond, cfg_strength=cfg, source=src)
        ref, nref = S.generate_latents_rk45(fresh, shape, cond=dcond, cfg_strength=cfg, source=src)
        assert torch.equal(got, ref) and ngot == nref
    else:
        S.generate_latents_rk45(model, shape, cond=dcond, cfg_strength=cfg, source=src)
        got, ngot, fgot = S.generate_latents_rk45(model, shape, cond=dcond, cfg_strength=cfg, source=src, t_eval=TE)
        ref, nref, fref = S.generate_latents_rk45(fresh, shape, cond=dcond, cfg_strength=cfg, source=src, t_eval=TE)
        assert torch.equal(got, ref) and ngot == nref and torch.equal(fgot, fref)


def test_t0_equal_t1_serves_the_source():
    z0, cond, cfg = _inputs("d16_cfg3")
    lat, counts, frames = _solve(_model("d16_cfg3"), z0, cond, cfg, False, [0.5], 0.5, 0.5)
    assert torch.equal(lat, z0) and counts.tolist() == [[1, 0, 0]] and torch.equal(frames[0], z0)


def test_frames_decode_like_latents():
    """The user's workflow: the trajectory at chosen times, decoded as one batch of F * B latents."""
    from flocoder_amd import sampling as S
    z0, cond, cfg = _inputs("d16_cfg3")

    class Codec(torch.nn.Module):
        def decode(self, z):
            return torch.nn.functional.interpolate(z[:, :3], scale_factor=2)

    lat, nfe, frames = S.generate_latents_rk45(_model("d16_cfg3"), tuple(z0.shape), cond=_dcond(cond), cfg_strength=cfg, source=z0.to(DEV),
                                               t_eval=TE)
    assert frames.shape == (len(TE), 2, 4, 16, 16) and frames.is_cuda and nfe > 2
    dec = S.decode_latents(Codec(), frames.flatten(0, 1))
    assert dec.shape == (len(TE) * 2, 3, 32, 32) and torch.isfinite(dec).all()
    assert torch.equal(dec[:2], Codec().decode(z0.to(DEV)))


_CHILD = r"""
import json, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import torch
from test_gpu_rk45_dense import GOLDEN, TE, _inputs, _model, _solve
from conftest import load_golden, rel_l2
g = load_golden(GOLDEN)
z0, cond, cfg = _inputs("d16_cfg3")
ref_f, ref_l = torch.from_numpy(g["coupled.d16_cfg3.frames"]), torch.from_numpy(g["coupled.d16_cfg3.latents"])
nfev_ref = int(g["coupled.d16_cfg3.counts"][0])
out = []
for te in (TE, None):
    lat, counts, frames = _solve(_model("d16_cfg3"), z0, cond, cfg, False, te)
    out.append(dict(dense=te is not None, rel_l2=rel_l2(lat, ref_l), nfev=int(counts[0, 0]), nfev_ref=nfev_ref,
                    frames=[rel_l2(frames[j], ref_f[j]) for j in range(len(TE))] if te is not None else [],
                    finite=bool(torch.isfinite(lat).all())))
print(json.dumps(dict(env=__import__("os").environ.get("AMD_DIRECT_DISPATCH"), calls=out)))
"""


@pytest.mark.skipif(os.environ.get("FLOCODER_AMD_IN_CHILD_SUITE") == "1", reason="already inside the child suite")
def test_dense_and_plain_calls_under_the_shipping_environment():
    """AMD_DIRECT_DISPATCH=0 (the mode the sampler ships with), a fresh process: one call with t_eval and one without on one handle, each
    against scipy + oracle.  Under this dispatch mode a graph replay has overtaken queued copies before (tests/test_gpu_shipping_env.py);
    the request record is such a copy."""
    env = {k: v for k, v in os.environ.items() if k != "FLOCODER_AMD_KEEP_ENV"}
    env["AMD_DIRECT_DISPATCH"] = "0"
    env["FLOCODER_AMD_IN_CHILD_SUITE"] = "1"
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    recs = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert r.returncode == 0 and recs, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    rec = recs[-1]
    assert rec["env"] == "0" and [c["dense"] for c in rec["calls"]] == [True, False]
    for c in rec["calls"]:
        assert c["finite"] and c["rel_l2"] < TRAJ_TOL and abs(c["nfev"] - c["nfev_ref"]) <= NFEV_SLACK, rec
        assert all(e < TRAJ_TOL for e in c["frames"]), rec
