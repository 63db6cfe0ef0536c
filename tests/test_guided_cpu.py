"""Measurement guidance on the CPU: ``inpainting.algorithm3`` against the reference's own outputs (tests/golden/g12_algorithm3.npz, made by
tools/make_golden_guided.py), its diagonal form against its dense form, and the generic-model path of
``sampling.generate_latents_guided`` against ``generate_latents_rk4`` and the fp64 restatement (tests/guided_ref.py).

Tolerances.  Golden cases: both sides are the same handful of fp64 operations and one well-conditioned k x k solve; the worst relative
difference measured here is 6.5e-16, the gate GOLDEN_TOL = 100 x that.  Diagonal against dense and the sampler against the restatement:
1e-12 relative, fp64 rounding of the same formulas in another operation order.  The last test holds the restatement itself to the
inequality tests/test_gpu_guided.py asks of the GPU, on that test's inputs."""
import pytest
import torch

import guided_ref as gr
from conftest import load_golden
from flocoder_amd import inpainting as I
from flocoder_amd import sampling as S
from oracle.synth import synth_input

GOLDEN_TOL = 6.5e-14        # 100 x the worst case measured (6.5e-16)
TRAJ_TOL = 2e-4             # tests/test_gpu_unet.py


def _rel(a, b):
    a, b = a.double().flatten(1), b.double().flatten(1)
    return (a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-300)


def test_dense_algorithm3_reproduces_the_references_outputs():
    g = load_golden("g12_algorithm3")
    v, x = torch.from_numpy(g["v"]), torch.from_numpy(g["x"])
    worst = 0.0
    assert len(g["case_tp"]) == 24
    for i, (kind, tp, sy, gam) in enumerate(zip(g["case_kind"], g["case_tp"], g["case_sigma_y"], g["case_gamma"])):
        A, y = torch.from_numpy(g[f"A_{kind}"]), torch.from_numpy(g[f"y_{kind}"])
        out = I.algorithm3(v, x, 0.0, float(tp), y, A, sigma_y=float(sy), gamma_t=float(gam))
        ref = torch.from_numpy(g[f"out_{i}"])
        assert out.dtype == torch.float64 and out.shape == x.shape
        err = float((out - ref).abs().max() / ref.abs().max())
        worst = max(worst, err)
        assert err <= GOLDEN_TOL, (i, kind, tp, sy, gam, err)
        assert float((out - v).abs().max()) > 1e-3            # the correction is there
    print(f"worst relative difference to the reference over 24 cases: {worst:.3e} (gate {GOLDEN_TOL:.1e})")


@pytest.mark.parametrize("sigma_y", [0.05, 0.5, 0.0])
@pytest.mark.parametrize("kind", ["binary", "fractional"])
def test_diagonal_form_equals_dense_form_with_zero_rows_dropped(kind, sigma_y):
    shape = (1, 4, 4, 4)
    v, x, known = (synth_input(f"guided.diag.{n}", shape, 5).double() for n in "vxk")
    u = torch.sigmoid(synth_input("guided.diag.a", shape, 5).double())
    a = (u > 0.45).double() if kind == "binary" else torch.where(u > 0.35, u, torch.zeros_like(u))
    assert 0 < int((a == 0).sum()) < a.numel()
    rows = torch.nonzero(a.flatten()).flatten()
    A = torch.diag(a.flatten())[rows]
    y_full = a * known
    for tp in (0.1, 0.5, 0.9):
        for gamma in (1.0, 0.5):
            d = I.algorithm3(v, x, 0.0, tp, y_full, a, sigma_y=sigma_y, gamma_t=gamma)
            e = I.algorithm3(v, x, 0.0, tp, y_full.flatten()[rows], A, sigma_y=sigma_y, gamma_t=gamma)
            assert torch.isfinite(d).all()
            assert float((d - e).abs().max()) <= 1e-12 * float(e.abs().max()), (tp, gamma)
            assert torch.equal(d[a == 0], v[a == 0])          # nothing measured there: v stays, also where sigma_y = 0 makes it 0/0
    # batched, with a [B,1,H,W] operator: every sample is its own problem
    vb, xb, kb = (synth_input(f"guided.diagb.{n}", (3, 4, 4, 4), 6).double() for n in "vxk")
    ab = (synth_input("guided.diagb.a", (3, 1, 4, 4), 6) > 0).double()
    full = I.algorithm3(vb, xb, 0.0, 0.4, ab * kb, ab, sigma_y=sigma_y)
    for b in range(3):
        one = I.algorithm3(vb[b:b + 1], xb[b:b + 1], 0.0, 0.4, (ab * kb)[b:b + 1], ab[b:b + 1].expand(1, 4, 4, 4), sigma_y=sigma_y)
        assert torch.equal(full[b:b + 1], one)


def test_ends_of_the_time_axis():
    shape = (2, 4, 4, 4)
    v, x, known = (synth_input(f"guided.ends.{n}", shape, 7).double() for n in "vxk")
    a = (synth_input("guided.ends.a", shape, 7) > 0).double()
    for sy in (0.05, 0.0):
        out = I.algorithm3(v, x, 0.0, 1.0, a * known, a, sigma_y=sy)
        assert torch.isfinite(out).all() and torch.equal(out, v)
    rows = torch.nonzero(a[:1].flatten()).flatten()
    A = torch.diag(a[:1].flatten())[rows]
    out = I.algorithm3(v[:1], x[:1], 0.0, 1.0, (a * known)[:1].flatten()[rows], A, sigma_y=0.05)
    assert torch.isfinite(out).all() and torch.equal(out, v[:1])
    for tp in (0.0, -0.1, torch.tensor(0.0)):
        with pytest.raises(ValueError, match="tp"):
            I.algorithm3(v, x, 0.0, tp, a * known, a)
    tiny = I.algorithm3(v, x, 0.0, 1e-6, a * known, a)
    assert torch.isfinite(tiny).all()


class _Field(torch.nn.Module):
    """A small analytic field with the model protocol: v = 0.3 conv(x) + cos(time / 999) x - 0.2 x^3 / (1 + x^2)."""

    def __init__(self, dtype):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.weight = torch.nn.Parameter(torch.randn(4, 4, 3, 3, generator=g, dtype=torch.float64).to(dtype) * 0.2, requires_grad=False)

    def forward(self, x, time, cond=None):
        t = (time / 999).view(-1, 1, 1, 1)
        return 0.3 * torch.nn.functional.conv2d(x, self.weight, padding=1) + torch.cos(t) * x - 0.2 * x ** 3 / (1 + x ** 2)


def _field_case(dtype):
    shape = (3, 4, 6, 6)
    src, known = synth_input("guided.f.src", shape, 8).to(dtype), synth_input("guided.f.known", shape, 8).to(dtype)
    keep = (synth_input("guided.f.keep", (3, 1, 6, 6), 8) > -0.2).to(dtype)
    return _Field(dtype), shape, src, known, keep


def test_generic_path_without_correction_is_the_plain_sampler():
    model, shape, src, known, keep = _field_case(torch.float32)
    y = keep * known
    for n, s in ((10, 0.2), (7, 0.5)):
        plain, nfe0 = S.generate_latents_rk4(model, shape, n, None, 3.0, source=src, init_latents=y, init_strength=s)
        for kw in (dict(keep=keep, gamma=0.0), dict(keep=torch.zeros_like(keep), gamma=1.0), dict(keep=torch.zeros(shape), gamma=1.0, sigma_y=0.0)):
            for jac in ("identity", "exact"):
                kk = dict(kw)
                lat, nfe = S.generate_latents_guided(model, shape, y, kk.pop("keep"), n_steps=n, init_strength=s, source=src, jacobian=jac, **kk)
                assert nfe == nfe0 and torch.equal(lat, plain), (n, s, kw.keys(), jac)
        lat, _ = S.generate_latents_guided(model, shape, y, keep, n_steps=n, init_strength=s, source=src)
        assert float(_rel(lat, plain).min()) > 1e-2               # and with it, it is another trajectory
    # init_latents other than the measurement
    other = synth_input("guided.f.init", shape, 9)
    plain, _ = S.generate_latents_rk4(model, shape, 10, None, 3.0, source=src, init_latents=other, init_strength=0.2)
    lat, _ = S.generate_latents_guided(model, shape, y, keep, n_steps=10, source=src, init_latents=other, gamma=0.0)
    assert torch.equal(lat, plain)


@pytest.mark.parametrize("jacobian", ["identity", "exact"])
def test_generic_path_equals_the_restatement_in_fp64(jacobian):
    model, shape, src, known, keep = _field_case(torch.float64)
    y = keep * known
    field = lambda x, t: model(x, torch.full((x.shape[0],), float(t), dtype=x.dtype) * 999)
    for sy, gam in ((0.05, 1.0), (0.5, 0.5)):
        lat, nfe = S.generate_latents_guided(model, shape, y, keep, n_steps=10, init_strength=0.2, source=src, sigma_y=sy, gamma=gam,
                                             jacobian=jacobian)
        start = 0.8 * src + 0.2 * y
        ts = S.rk4_time_grid(10, 0.2, dtype=torch.float64)
        ref = gr.guided_rk4(field, start, ts, y, keep, sy, gam, jacobian == "exact")
        assert nfe == 32 and len(ref.stages) == 28 and lat.dtype == torch.float64
        assert float(_rel(lat, ref.latents).max()) <= 1e-12
    ident = gr.guided_rk4(field, start, ts, y, keep, sy, gam, False).latents
    if jacobian == "exact":
        assert float(_rel(lat, ident).min()) > 1e-3               # the Jacobian term is live in the torch path


def test_argument_errors():
    model, shape, src, known, keep = _field_case(torch.float32)
    y = keep * known
    for s in (0.0, -0.1, None):
        with pytest.raises(ValueError, match="init_strength"):
            S.generate_latents_guided(model, shape, y, keep, init_strength=s, source=src)
    with pytest.raises(ValueError, match="guidance"):
        S.generate_latents_guided(model, shape, y, keep, source=src, cond={"class_cond": torch.tensor([0, 1, 2])}, cfg_strength=3.0,
                                  jacobian="exact")
    S.generate_latents_guided(model, shape, y, keep, n_steps=4, source=src, cond={"class_cond": torch.tensor([0, 1, 2])}, cfg_strength=0.0,
                              jacobian="exact")
    with pytest.raises(ValueError, match="jacobian"):
        S.generate_latents_guided(model, shape, y, keep, source=src, jacobian="autograd")
    with pytest.raises(ValueError, match="sigma_y"):
        S.generate_latents_guided(model, shape, y, keep, source=src, sigma_y=-1.0)
    with pytest.raises(ValueError, match="measurement"):
        S.generate_latents_guided(model, shape, y[:, :2], keep, source=src)
    with pytest.raises(ValueError, match="keep"):
        S.generate_latents_guided(model, shape, y, keep[:, :, :3], source=src)
    from flocoder_amd.unet import Unet
    m = Unet(dim=8, channels=4, n_classes=0).eval()
    z = torch.zeros(1, 4, 8, 8)
    with pytest.raises(RuntimeError, match="MI355X"):
        S.generate_latents_guided(m, (1, 4, 8, 8), z, torch.ones(1, 1, 8, 8), n_steps=4, source=z)


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("cid", list(gr.CASES))
def test_the_restatement_satisfies_the_gpu_tests_inequalities_on_its_inputs(cid):
    """What tests/test_gpu_guided.py asks of the GPU samples must hold for the fp64 restatement on the same inputs first: the kept-region
    residual of the guided sample is below the unguided one's for every sample, and the exact form is a different trajectory from the
    identity form (without classifier-free guidance) by more than the trajectory tolerance."""
    c = gr.case_inputs(cid)
    which = ("identity", "exact", "unguided") + (("identity0",) if c["cfg"] else ())
    refs = gr.case_refs(cid, which)
    r_g = gr.kept_residual(refs["identity"].latents, c["keep"], c["known"])
    r_e = gr.kept_residual(refs["exact"].latents, c["keep"], c["known"])
    r_u = gr.kept_residual(refs["unguided"], c["keep"], c["known"])
    ident0 = refs["identity0" if c["cfg"] else "identity"].latents
    diff = _rel(refs["exact"].latents, ident0)
    print(f"\n[{cid}] kept-region residual: guided {r_g.tolist()}, exact {r_e.tolist()}, unguided {r_u.tolist()}; exact vs identity rel-L2 {diff.tolist()}")
    assert torch.isfinite(refs["identity"].latents).all() and torch.isfinite(refs["exact"].latents).all()
    assert bool((r_g < r_u).all()), (r_g, r_u)
    assert float(diff.min()) > TRAJ_TOL, diff
