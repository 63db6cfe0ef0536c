"""Adaptive RK45 sampler (legacy/train_sd_flowers.py:78-107; the reference's generate_latents(method="rk45") dispatch, sampling.py:142-143)
on the host: a plain torch field goes through scipy exactly as the legacy code does, and the argument checks hold without a GPU."""
import warnings

import numpy as np
import pytest
import torch
from torch import nn

from flocoder_amd import sampling as S


class SinField(nn.Module):
    """v = -x + sin(t), t = time / 999 as the samplers hand it over."""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.ones(()))

    def forward(self, x, time, cond=None):
        t = (time / 999.0).view(-1, 1, 1, 1)
        return self.w * (-x) + torch.sin(t)


def _legacy_rk45(model, z0, eps=1e-3, rtol=1e-5, atol=1e-5):
    """rk45_sampler of train_sd_flowers.py:78-107 with the noise supplied (no class conditioning)."""
    from scipy import integrate
    shape = tuple(z0.shape)

    def ode_func(t, x):
        x = torch.from_numpy(x.reshape(shape)).type(torch.float32)
        vec_t = torch.ones(shape[0]) * t
        return model(x, vec_t * 999, None).detach().cpu().numpy().reshape((-1,))

    sol = integrate.solve_ivp(ode_func, (eps, 1), z0.detach().cpu().numpy().reshape((-1,)), rtol=rtol, atol=atol, method="RK45")
    return torch.tensor(sol.y[:, -1]).reshape(shape).type(torch.float32), sol.nfev


def test_generate_latents_rk45_matches_scipy_on_a_plain_field():
    model = SinField()
    z0 = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(3))
    lat, nfe = S.generate_latents(model, tuple(z0.shape), method="rk45", source=z0)
    ref, ref_nfe = _legacy_rk45(model, z0)
    assert nfe == ref_nfe and nfe > 2 and (nfe - 2) % 6 == 0
    assert torch.equal(lat, ref)
    # and the field is integrated: x(1) = e^-(1-eps) x(eps) + the particular solution
    assert float((lat - z0).abs().max()) > 0.1


def test_rk45_sampler_class_ids_and_cfg_on_a_plain_field():
    class Cond(SinField):
        def forward(self, x, time, cond=None):
            v = super().forward(x, time)
            if cond and cond.get("class_cond") is not None:
                v = v + cond["class_cond"].float().view(-1, 1, 1, 1)
            return v

    model = Cond()
    z0 = torch.randn(2, 4, 4, 4, generator=torch.Generator().manual_seed(4))
    ids = torch.tensor([1, 2])
    a, na = S.rk45_sampler(model, tuple(z0.shape), cond=ids, source=z0)
    b, nb = S.rk45_sampler(model, tuple(z0.shape), cond={"class_cond": ids}, source=z0, cfg_strength=2.0)
    # guided field: v_nc + 2 (v_c - v_nc) = sin field + 2 ids, integrated over (1e-3, 1)
    assert na > 0 and nb > 0
    assert torch.allclose(b - a, (2 - 1) * (1 - torch.exp(torch.tensor(-(1 - 1e-3)))) * ids.float().view(-1, 1, 1, 1).expand_as(a), atol=1e-4)


def test_unet_on_cpu_has_no_cpu_path():
    from flocoder_amd.unet import Unet
    torch.manual_seed(0)
    m = Unet(dim=8, dim_mults=(1, 2), channels=4, n_classes=0).eval()
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.generate_latents(m, (1, 4, 8, 8), method="rk45", source=torch.zeros(1, 4, 8, 8))


def test_negative_atol_raises():
    with pytest.raises(ValueError, match="atol"):
        S.rk45_sampler(SinField(), (1, 4, 4, 4), source=torch.zeros(1, 4, 4, 4), atol=-1e-5)


def test_tiny_rtol_is_raised_with_a_warning():
    z0 = torch.ones(1, 4, 2, 2)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        S.rk45_sampler(SinField(), tuple(z0.shape), source=z0, rtol=0.0, atol=1e-3)
    assert any("rtol" in str(x.message) for x in w)


def test_init_latents_with_rk45_raises():
    z0 = torch.zeros(1, 4, 4, 4)
    with pytest.raises(ValueError, match="init_latents"):
        S.generate_latents(SinField(), tuple(z0.shape), method="rk45", source=z0, init_latents=z0, init_strength=0.5)


def test_sampler_rk45_returns_nfe():
    class Codec(nn.Module):
        def decode(self, z):
            return z * 2

    z0 = torch.randn(2, 4, 4, 4, generator=torch.Generator().manual_seed(5))
    lat, dec, nfe = S.sampler(SinField(), Codec(), method="rk45", batch_size=2, latent_shape=(4, 4, 4), source=z0, device=torch.device("cpu"))
    ref, ref_nfe = _legacy_rk45(SinField(), z0)
    assert nfe == ref_nfe and torch.equal(lat, ref) and torch.equal(dec, 2 * ref)
    assert np.isfinite(dec.numpy()).all()
