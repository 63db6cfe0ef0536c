"""Stochastic (SDE) sampling without a GPU: the counter-based normal field (flocoder_amd/noise.py) and the torch path of
sampling.generate_latents_sde against tests/sde_ref.py.

  field        Philox4x32-10 known answers (Random123's vectors); a sample's normals depend on (seed, draw, sample id) alone; moments and
               correlations of 2^22 values within 5 standard errors
  marginals    on the exact velocity field between N(0,1) and N(2, 0.5^2) the SDE must END in N(2, 0.5^2) for every sigma: Heun at 51 grid
               points within 5 standard errors of mean and std (409 600 elements); Euler-Maruyama's std error falls first order
  restatement  the generic path equals sde_ref given the same field values (fp64, 1e-12)
"""
import numpy as np
import pytest
import torch

import sde_ref as sr
from flocoder_amd import noise as N
from flocoder_amd import sampling as S
from oracle.synth import synth_input

KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def _rel(a, b):
    a, b = a.double().flatten(1), b.double().flatten(1)
    return (a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-300)


def test_philox_known_answers():
    for ctr, key, want in KAT:
        got = N.philox4x32(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert " ".join(f"{int(w):08x}" for w in got) == want
    both = N.philox4x32(np.array([k[0] for k in KAT], dtype=np.uint64), np.array([k[1] for k in KAT], dtype=np.uint64))     # vectorised
    assert [" ".join(f"{int(w):08x}" for w in row) for row in both] == [k[2] for k in KAT]


def test_counter_layout_and_uniforms():
    """Word k of block j of (seed, draw, id) is philox(ctr = (j, draw, id lo, id hi), key = (seed lo, seed hi)); the uniforms are fp32
    numbers in (0, 1); the normals follow the documented Box-Muller pairs."""
    seed, draw, sid = (0x12345678 << 32) | 0x9abcdef0, 7, (5 << 32) | 11
    w = N.field_words(seed, draw, [sid], 16)
    assert w.shape == (1, 4, 4) and w.dtype == np.uint32
    for j in range(4):
        one = N.philox4x32(np.array([j, draw, 11, 5], dtype=np.uint64), np.array([0x9abcdef0, 0x12345678], dtype=np.uint64))
        assert (w[0, j] == one).all()
    u = N.uniforms(w)
    assert (u > 0).all() and (u < 1).all() and (u.astype(np.float32).astype(np.float64) == u).all()
    z = N.normal_field(seed, draw, [sid], 16)[0].reshape(4, 4)
    r0 = np.sqrt(-2 * np.log(u[0, :, 0]))
    assert np.allclose(z[:, 0], r0 * np.cos(2 * np.pi * u[0, :, 1]), rtol=0, atol=1e-14)
    assert np.allclose(z[:, 3], np.sqrt(-2 * np.log(u[0, :, 2])) * np.sin(2 * np.pi * u[0, :, 3]), rtol=0, atol=1e-14)
    assert abs(z).max() <= N.TAIL and abs(N.TAIL - np.sqrt(48 * np.log(2))) < 1e-12
    assert N.normal_field(seed, draw, [-3], 8).shape == (1, 8)                    # a negative id is its two's complement
    with pytest.raises(ValueError):
        N.normal_field(0, 0, [0], 6)
    with pytest.raises(ValueError):
        N.normal_field(0, -1, [0], 8)


def test_a_samples_normals_do_not_depend_on_its_batch():
    per = 4 * 8 * 8
    ids = np.array([5, 0, 17, 2 ** 40 + 3], dtype=np.int64)
    whole = N.normal_field(9, 3, ids, per)
    for b, sid in enumerate(ids):
        assert np.array_equal(N.normal_field(9, 3, [sid], per)[0], whole[b])
    perm = np.array([2, 3, 0, 1])
    assert np.array_equal(N.normal_field(9, 3, ids[perm], per), whole[perm])
    assert np.array_equal(N.normal_field(9, 3, np.arange(6), per)[:3], N.normal_field(9, 3, np.arange(3), per))
    base = N.normal_field(9, 3, [5], per)
    for other in (N.normal_field(10, 3, [5], per), N.normal_field(9, 4, [5], per), N.normal_field(9, 3, [6], per),
                  N.normal_field(9 + 2 ** 32, 3, [5], per), N.normal_field(9, 3, [5 + 2 ** 32], per)):
        assert not np.array_equal(other, base) and abs(np.corrcoef(other[0], base[0])[0, 1]) < 5 / np.sqrt(per)


def test_moments_and_correlations_of_the_field():
    B_, per = 64, 65536
    n = B_ * per                                                     # 2^22
    z = N.normal_field(1234, 0, np.arange(B_), per)
    z1 = N.normal_field(1234, 1, np.arange(B_), per)                 # the next draw of the same samples
    mean, var, m4 = z.mean(), (z ** 2).mean(), (z ** 4).mean()
    print(f"\nN = {n}: mean {mean:.3e} (5 se {5 / np.sqrt(n):.3e}), E z^2 - 1 {var - 1:.3e} (5 se {5 * np.sqrt(2 / n):.3e}), "
          f"E z^4 - 3 {m4 - 3:.3e} (5 se {5 * np.sqrt(96 / n):.3e}), max |z| {abs(z).max():.3f}")
    assert abs(mean) < 5 / np.sqrt(n)
    assert abs(var - 1) < 5 * np.sqrt(2 / n)
    assert abs(m4 - 3) < 5 * np.sqrt(96 / n)
    c_draw = (z * z1).mean()
    c_ids = (z[:-1] * z[1:]).mean()
    c_pair = (z[:, 0::2] * z[:, 1::2]).mean()                        # the cos / sin halves of a Box-Muller pair
    print(f"correlation: consecutive draws {c_draw:.3e}, neighbouring ids {c_ids:.3e}, pair halves {c_pair:.3e} (5 / sqrt N {5 / np.sqrt(n):.3e})")
    assert abs(c_draw) < 5 / np.sqrt(n)
    assert abs(c_ids) < 5 / np.sqrt(n - per)
    assert abs(c_pair) < 5 / np.sqrt(n / 2)


# ------------------------------------------------------------------------------------------- marginals on the analytic flow
M, SD = 2.0, 0.5
GAUSS_SHAPE = (100, 4, 32, 32)


def _gauss_run(n_points, sigma, method, seed=11):
    src = torch.randn(GAUSS_SHAPE, generator=torch.Generator().manual_seed(42), dtype=torch.float64)
    lat, nfe = S.generate_latents_sde(sr.GaussianFlow(torch.float64, M, SD), GAUSS_SHAPE, n_steps=n_points, cfg_strength=0.0, source=src,
                                      sigma=sigma, method=method, seed=seed)
    assert lat.dtype == torch.float64 and nfe == (n_points - 1) * (2 if method == "heun" else 1)
    return lat


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("sigma", [0.0, 1.0, 2.0])
def test_heun_ends_in_the_data_distribution(sigma):
    lat = _gauss_run(51, sigma, "heun")
    n = lat.numel()
    mean, std = float(lat.mean()), float(lat.std())
    print(f"\nsigma = {sigma}: mean {mean:.5f} (band {5 * SD / np.sqrt(n):.5f}), std {std:.5f} (band {5 * SD / np.sqrt(2 * n):.5f})")
    assert n == 409600
    assert abs(mean - M) < 5 * SD / np.sqrt(n)
    assert abs(std - SD) < 5 * SD / np.sqrt(2 * n)


@pytest.mark.timeout(1800)
def test_euler_maruyama_is_first_order_in_the_marginal_std():
    errs = [abs(float(_gauss_run(n, 1.0, "euler_maruyama").std()) - SD) for n in (26, 51, 101)]
    print(f"\nEuler-Maruyama |std - {SD}| at 26 / 51 / 101 points: {errs}")
    for coarse, fine in zip(errs, errs[1:]):
        assert 1.6 < coarse / fine < 2.6, errs


# ------------------------------------------------------------------------------------------- the generic path against the restatement
class _Field(torch.nn.Module):
    """A small analytic field with the model protocol: v = 0.3 conv(x) + cos(time / 999) x - 0.2 x^3 / (1 + x^2) (+ 0.1 class id)."""

    def __init__(self, dtype):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.weight = torch.nn.Parameter(torch.randn(4, 4, 3, 3, generator=g, dtype=torch.float64).to(dtype) * 0.2, requires_grad=False)

    def forward(self, x, time, cond=None):
        t = (time / 999).view(-1, 1, 1, 1)
        v = 0.3 * torch.nn.functional.conv2d(x, self.weight, padding=1) + torch.cos(t) * x - 0.2 * x ** 3 / (1 + x ** 2)
        if cond and cond.get("class_cond") is not None:
            v = v + 0.1 * cond["class_cond"].to(x.dtype).view(-1, 1, 1, 1)
        return v


SHAPE = (3, 4, 6, 6)


def _case(dtype):
    return _Field(dtype), synth_input("sde.f.src", SHAPE, 8).to(dtype)


def _as_field(model, cond=None, cfg=0.0):
    def field(x, t):
        tv = torch.full((x.shape[0],), float(t), dtype=x.dtype) * 999
        v = model(x, tv, cond=cond)
        if cond and cond.get("class_cond") is not None and cfg:
            vn = model(x, tv, cond={"class_cond": None})
            v = vn + cfg * (v - vn)
        return v
    return field


def _field_noise(seed, ids, n_int, dtype=torch.float64):
    per = SHAPE[1] * SHAPE[2] * SHAPE[3]
    return torch.stack([torch.from_numpy(N.normal_field(seed, i, ids, per)).reshape(SHAPE) for i in range(n_int)]).to(dtype)


@pytest.mark.parametrize("method", sr.SCHEMES)
def test_generic_path_equals_the_restatement_in_fp64(method):
    model, src = _case(torch.float64)
    ts = S.rk4_time_grid(10, dtype=torch.float64)
    k = 2 if method == "heun" else 1
    for sigma, seed, ids in ((1.0, 0, None), (0.5, 2 ** 40 + 7, torch.tensor([4, 9, 1]))):
        lat, nfe = S.generate_latents_sde(model, SHAPE, n_steps=10, cfg_strength=0.0, source=src, sigma=sigma, method=method, seed=seed,
                                          sample_ids=ids)
        xi = _field_noise(seed, np.arange(3) if ids is None else ids.numpy(), 9)
        ref = sr.sde_solve(_as_field(model), src, ts, sigma, method, xi)
        assert nfe == 9 * k and lat.dtype == torch.float64
        assert float(_rel(lat, ref).max()) <= 1e-12
        # supplied noise equal to the generated field gives the generated run's result
        sup, _ = S.generate_latents_sde(model, SHAPE, n_steps=10, cfg_strength=0.0, source=src, sigma=sigma, method=method, noise=xi)
        assert torch.equal(sup, lat)
    # classifier-free guidance and init_latents: RK4's start and grid
    cond = {"class_cond": torch.tensor([1, 3, 7])}
    init = synth_input("sde.f.init", SHAPE, 9).double()
    lat, nfe = S.generate_latents_sde(model, SHAPE, n_steps=12, cond=cond, cfg_strength=3.0, source=src, init_latents=init, init_strength=0.25,
                                      sigma=1.0, method=method, seed=5)
    ts = S.rk4_time_grid(12, 0.25, dtype=torch.float64)
    assert len(ts) == 9 and nfe == 8 * k
    ref = sr.sde_solve(_as_field(model, cond, 3.0), 0.75 * src + 0.25 * init, ts, 1.0, method, _field_noise(5, np.arange(3), 8))
    assert float(_rel(lat, ref).max()) <= 1e-12
    assert float(_rel(lat, S.generate_latents_sde(model, SHAPE, n_steps=12, cond=cond, cfg_strength=0.0, source=src, init_latents=init,
                                                  init_strength=0.25, sigma=1.0, method=method, seed=5)[0]).min()) > 1e-3


@pytest.mark.parametrize("method", sr.SCHEMES)
def test_seeds_ids_and_sigma_zero(method):
    model, src = _case(torch.float32)
    run = lambda **kw: S.generate_latents_sde(model, SHAPE, n_steps=8, cfg_strength=0.0, source=src, method=method, **kw)[0]
    a, b = run(sigma=0.0, seed=1), run(sigma=0.0, seed=2)
    assert torch.equal(a, b)                                         # no diffusion: the seed is not in the result
    ts = S.rk4_time_grid(8)
    det = sr.sde_solve(_as_field(model), src, ts, 0.0, method, torch.zeros((7,) + SHAPE))
    assert float(_rel(a, det).max()) < 1e-6
    s1, s1b, s2 = run(sigma=1.0, seed=1), run(sigma=1.0, seed=1), run(sigma=1.0, seed=2)
    assert torch.equal(s1, s1b) and float(_rel(s2, s1).min()) > 1e-2 and torch.isfinite(s1).all()
    # a row follows its sample id, not its position
    ids = torch.tensor([2, 0, 1])
    moved = S.generate_latents_sde(model, SHAPE, n_steps=8, cfg_strength=0.0, source=src[ids], method=method, sigma=1.0, seed=1,
                                   sample_ids=ids)[0]
    assert float(_rel(moved, s1[ids]).max()) < 1e-5                  # (the convolution's batch blocking may differ in the last bit)


def test_dispatch_and_argument_errors():
    model, src = _case(torch.float32)
    for name, method in (("sde", "euler_maruyama"), ("sde_heun", "heun")):
        a, na = S.generate_latents(model, SHAPE, method=name, n_steps=6, cfg_strength=0.0, source=src, sigma=0.7, seed=3)
        b, nb = S.generate_latents_sde(model, SHAPE, n_steps=6, cfg_strength=0.0, source=src, sigma=0.7, seed=3, method=method)
        assert torch.equal(a, b) and na == nb == 5 * (2 if method == "heun" else 1)
    with pytest.raises(TypeError):
        S.generate_latents(model, SHAPE, method="rk4", n_steps=6, source=src, sigma=0.7)
    kw = dict(n_steps=6, cfg_strength=0.0, source=src)
    with pytest.raises(ValueError, match="sigma"):
        S.generate_latents_sde(model, SHAPE, sigma=-0.1, **kw)
    with pytest.raises(ValueError, match="method"):
        S.generate_latents_sde(model, SHAPE, method="milstein", **kw)
    with pytest.raises(ValueError, match="noise"):
        S.generate_latents_sde(model, SHAPE, noise=torch.zeros((6,) + SHAPE), **kw)             # 5 intervals
    with pytest.raises(ValueError, match="sample_ids"):
        S.generate_latents_sde(model, SHAPE, sample_ids=torch.tensor([0, 1]), **kw)
    with pytest.raises(ValueError, match="sample_ids"):
        S.generate_latents_sde(model, SHAPE, sample_ids=torch.tensor([0, 1, 2], dtype=torch.int32), **kw)
    with pytest.raises(ValueError, match="two points"):
        S.generate_latents_sde(model, SHAPE, n_steps=1, cfg_strength=0.0, source=src)
    from flocoder_amd.unet import Unet
    m = Unet(dim=8, channels=4, n_classes=0).eval()
    z = torch.zeros(1, 4, 8, 8)
    with pytest.raises(RuntimeError, match="MI355X"):
        S.generate_latents_sde(m, (1, 4, 8, 8), n_steps=4, source=z)
    with pytest.raises(RuntimeError, match="MI355X"):
        m.integrate_sde(z, S.rk4_time_grid(4), sigma=1.0, method="heun")
    with pytest.raises(ValueError, match="method"):
        m.integrate_sde(z, S.rk4_time_grid(4), sigma=1.0, method="rk4")
    with pytest.raises(ValueError, match="sigma"):
        m.integrate_sde(z, S.rk4_time_grid(4), sigma=-1.0, method="heun")
