"""Restatement of stochastic (SDE) sampling (flocoder_amd.sampling.generate_latents_sde) over the oracle U-Net or any callable field (test
helper, imported by tests/test_sde_cpu.py and tests/test_gpu_sde.py; not a conftest).

Written from the formulas of DESIGN.md section 4b, not from the code under test, in the dtype of the inputs (fp64 for the yardstick).  On
the linear path x_t = (1-t) x0 + t x1, x0 ~ N(0, I), with diffusion sigma^2 (1-t) the SDE that keeps the ODE's marginals is

    dx = b(x,t) dt + sigma sqrt(1-t) dW          b(x,t) = (1 + sigma^2 t / 2) v(x,t) - (sigma^2 / 2) x

and on interval i of the grid, h = t_{i+1} - t_i, a_i = sigma sqrt(h (1 - (t_i + t_{i+1})/2)), xi_i the interval's noise:

    euler_maruyama    x+ = x + h b(x,t_i) + a_i xi_i
    heun              xp = x + h b(x,t_i) + a_i xi_i ;   x+ = x + (h/2) (b(x,t_i) + b(xp,t_{i+1})) + a_i xi_i

``v`` is the velocity after classifier-free guidance (``flow_oracle.velocity_cfg``).  Start and grid as ``flow_oracle.generate_latents_rk4``.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch

from oracle import flow_oracle as fo

import guided_ref as gr

SCHEMES = ("euler_maruyama", "heun")


def drift(field: Callable, x, t, sigma):
    return (1 + 0.5 * sigma * sigma * t) * field(x, t) - 0.5 * sigma * sigma * x


def noise_scale(t0, t1, sigma):
    """Standard deviation of the integral of sigma sqrt(1-t) dW over [t0, t1]: sigma^2 (1-t) is linear, its integral is h (1 - midpoint)."""
    return sigma * torch.sqrt((t1 - t0) * (1 - (t0 + t1) / 2))


def sde_solve(field: Callable, start, ts, sigma: float, scheme: str, noise) -> torch.Tensor:
    """``noise``: a tensor [len(ts)-1, *start.shape] or a callable i -> tensor of start's shape."""
    assert scheme in SCHEMES
    x = start.detach()
    with torch.no_grad():
        for i in range(len(ts) - 1):
            t0, t1 = ts[i], ts[i + 1]
            h = t1 - t0
            kick = noise_scale(t0, t1, sigma) * (noise(i) if callable(noise) else noise[i]).to(x.dtype)
            b0 = drift(field, x, t0, sigma)
            if scheme == "euler_maruyama":
                x = x + h * b0 + kick
            else:
                xp = x + h * b0 + kick
                x = x + (h / 2) * (b0 + drift(field, xp, t1, sigma)) + kick
    return x


def sde_ref(sd, source, n_steps: int, cond: Optional[dict], cfg_strength: float, sigma: float, scheme: str, noise, init_latents=None,
            init_strength: float = 0.0) -> torch.Tensor:
    """generate_latents_sde over the oracle U-Net with state dict ``sd``, in the dtype of ``source``."""
    dtype = source.dtype
    if init_latents is None:
        start, ts = source, fo.rk4_time_grid(n_steps, dtype)
    else:
        start = (1 - init_strength) * source + init_strength * init_latents.to(dtype)
        ts = fo.rk4_time_grid(n_steps, dtype, init_strength=init_strength)
    field = lambda x, t: fo.velocity_cfg(sd, cond, cfg_strength, x, t)
    return sde_solve(field, start, ts, sigma, scheme, noise)


# ------------------------------------------------------------------------------------------- the analytic flow of the marginal test
def gaussian_velocity(x, t, m: float = 2.0, s: float = 0.5):
    """The exact velocity of the linear path from N(0, 1) to N(m, s^2), per element: x_t ~ N(t m, (1-t)^2 + t^2 s^2) and
    v = E[x1 - x0 | x_t] = m + (t s^2 - (1-t)) / ((1-t)^2 + t^2 s^2) (x - t m)."""
    return m + (t * s * s - (1 - t)) / ((1 - t) ** 2 + t * t * s * s) * (x - t * m)


class GaussianFlow(torch.nn.Module):
    """``gaussian_velocity`` with the model protocol ``model(x, 999 t, cond=None)``; its one (unused) parameter tells the samplers its
    device and dtype."""

    def __init__(self, dtype=torch.float64, m: float = 2.0, s: float = 0.5):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros((), dtype=dtype), requires_grad=False)
        self.m, self.s = m, s

    def forward(self, x, time, cond=None):
        t = (time / 999).view(-1, *([1] * (x.dim() - 1)))
        return gaussian_velocity(x, t, self.m, self.s)


# ------------------------------------------------------------------------------------------- the GPU test's cases
# tests/guided_ref.py CASES (the likelihood test's models): id -> model, batch, size, conditioning, cfg_strength, n_steps.  sigma = 1.
SIGMA = 1.0
CASES = gr.CASES


def case_inputs(cid):
    """-> dict(sd, source, cond, cfg, n, noise): fp32 CPU tensors; ``noise`` [n-1, B, 4, H, W] standard normal from a torch generator."""
    c = gr.case_inputs(cid)
    g = torch.Generator().manual_seed(7000 + len(cid))
    noise = torch.randn((c["n"] - 1,) + tuple(c["source"].shape), generator=g)
    return dict(sd=c["sd"], source=c["source"], cond=c["cond"], cfg=c["cfg"], n=c["n"], noise=noise)


def case_ref(cid, scheme, cfg, sigma=SIGMA, noise=None):
    """The fp64 restatement of a case at guidance ``cfg`` -> latents."""
    c = case_inputs(cid)
    sd64 = {k: v.double() for k, v in c["sd"].items()}
    nz = c["noise"] if noise is None else noise
    return sde_ref(sd64, c["source"].double(), c["n"], c["cond"], cfg, sigma, scheme, nz.double())
