"""Per-sample adaptive RK45 (generate_latents(method="rk45_per_sample"), rk45_sampler(per_sample=True)) on the host: every sample is its
own scipy solve_ivp(method="RK45") problem, so a plain torch field whose samples differ in stiffness gives each sample the result and the
counters of an independent solve on that sample alone, whatever its batchmates are."""
import pytest
import torch
from torch import nn

from flocoder_amd import sampling as S


class StiffField(nn.Module):
    """v = -k x + sin(t), with a per-sample decay rate k = 1 + 4 * class id (t = time / 999 as the samplers hand it over)."""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.ones(()))

    def forward(self, x, time, cond=None):
        t = (time / 999.0).view(-1, 1, 1, 1)
        k = 1.0 + 4.0 * cond["class_cond"].float().view(-1, 1, 1, 1)
        return self.w * (-k * x) + torch.sin(t)


def _solo(model, z0, ids, eps=1e-3, rtol=1e-5, atol=1e-5):
    """scipy on each sample alone: (latents, [nfev per sample])."""
    from scipy import integrate
    lats, nfevs = [], []
    for b in range(z0.shape[0]):
        shape = (1,) + tuple(z0.shape[1:])
        cond = {"class_cond": ids[b:b + 1]}

        def f(t, y):
            x = torch.from_numpy(y.reshape(shape)).type(torch.float32)
            return model(x, torch.ones(1) * t * 999, cond).detach().numpy().reshape(-1)

        sol = integrate.solve_ivp(f, (eps, 1), z0[b].numpy().reshape(-1), rtol=rtol, atol=atol, method="RK45")
        assert sol.success
        lats.append(torch.tensor(sol.y[:, -1]).reshape(shape).type(torch.float32))
        nfevs.append(int(sol.nfev))
    return torch.cat(lats), nfevs


def _inputs():
    z0 = torch.randn(3, 4, 4, 4, generator=torch.Generator().manual_seed(21))
    return z0, torch.tensor([0, 3, 9])


def test_each_sample_is_its_own_scipy_solve():
    model = StiffField()
    z0, ids = _inputs()
    lat, nfe = S.generate_latents(model, tuple(z0.shape), method="rk45_per_sample", cond={"class_cond": ids}, cfg_strength=0.0,
                                  source=z0)
    ref, nfevs = _solo(model, z0, ids)
    assert torch.equal(lat, ref)
    assert nfe == max(nfevs)
    # the samples really run separate controllers: their step counts differ
    assert len(set(nfevs)) == len(nfevs), nfevs


def test_sampler_and_per_sample_flag_agree():
    model = StiffField()
    z0, ids = _inputs()
    a, na = S.rk45_sampler(model, tuple(z0.shape), cond=ids, source=z0, per_sample=True)
    b, nb = S.generate_latents_rk45(model, tuple(z0.shape), cond={"class_cond": ids}, cfg_strength=0.0, source=z0, per_sample=True)
    assert torch.equal(a, b) and na == nb


def test_a_sample_does_not_depend_on_its_batchmates():
    model = StiffField()
    z0, ids = _inputs()
    lat, _ = S.generate_latents(model, tuple(z0.shape), method="rk45_per_sample", cond={"class_cond": ids}, cfg_strength=0.0, source=z0)
    z1 = z0.clone()
    z1[1] = 5.0 * torch.randn(z0.shape[1:], generator=torch.Generator().manual_seed(22))
    lat1, _ = S.generate_latents(model, tuple(z1.shape), method="rk45_per_sample", cond={"class_cond": ids}, cfg_strength=0.0, source=z1)
    assert torch.equal(lat1[0], lat[0]) and torch.equal(lat1[2], lat[2])
    assert not torch.equal(lat1[1], lat[1])
    # and a batch of one gives the same sample
    one, _ = S.generate_latents(model, (1,) + tuple(z0.shape[1:]), method="rk45_per_sample", cond={"class_cond": ids[:1]},
                                cfg_strength=0.0, source=z0[:1])
    assert torch.equal(one[0], lat[0])


def test_batch_coupled_mode_differs():
    """The default "rk45" solves the batch as one system: one step size for all, so its result is not the per-sample one."""
    model = StiffField()
    z0, ids = _inputs()
    lat, _ = S.generate_latents(model, tuple(z0.shape), method="rk45_per_sample", cond={"class_cond": ids}, cfg_strength=0.0, source=z0)
    coupled, _ = S.generate_latents(model, tuple(z0.shape), method="rk45", cond={"class_cond": ids}, cfg_strength=0.0, source=z0)
    assert not torch.equal(lat, coupled)


def test_negative_atol_raises():
    z0, ids = _inputs()
    with pytest.raises(ValueError, match="atol"):
        S.rk45_sampler(StiffField(), tuple(z0.shape), cond=ids, source=z0, atol=-1e-5, per_sample=True)


def test_init_latents_with_rk45_per_sample_raises():
    z0, ids = _inputs()
    with pytest.raises(ValueError, match="init_latents"):
        S.generate_latents(StiffField(), tuple(z0.shape), method="rk45_per_sample", cond={"class_cond": ids}, source=z0, init_latents=z0,
                           init_strength=0.5)


def test_a_failing_sample_is_named():
    class Blowup(StiffField):
        def forward(self, x, time, cond=None):
            v = super().forward(x, time, cond)
            bad = (cond["class_cond"] == 7).float().view(-1, 1, 1, 1)
            return v + bad * 1e30 * x * x          # sample with class 7 explodes in finite time

    z0 = torch.ones(2, 4, 2, 2)
    with pytest.raises(RuntimeError, match="sample 1"):
        S.rk45_sampler(Blowup(), tuple(z0.shape), cond=torch.tensor([0, 7]), source=z0, per_sample=True)
