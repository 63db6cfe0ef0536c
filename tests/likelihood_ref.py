"""Restatement of the flow log-likelihood / latent inversion on the reversed RK4 grid over the oracle U-Net (test helper, imported by
tests/test_likelihood_cpu.py and tests/test_gpu_likelihood.py; not a conftest).

``oracle.flow_oracle.unet_forward`` under autograd, in the dtype of the state dict (fp64 for the yardstick).  Semantics, as
``flocoder_amd.sampling.log_likelihood`` documents them: ``ts = rk4_time_grid(n_steps)`` walked backwards; per interval the four RK4
stages, each with ``g_j = (dv_j/dx_j)^T eps`` and ``d_j[b] = sum_i eps[b,i] g_j[b,i]`` (fp64 products and sum);

    x <- x + (dt/6)(v1 + 2 v2 + 2 v3 + v4)        a <- a + (dt/6)(d1 + 2 d2 + 2 d3 + d4)        logp = -|z|^2/2 - (D/2) ln 2pi + a

Besides the results every stage is recorded (state, time, g_j, d_j), and ``gsum[b] = sum over intervals of (|dt|/6)(|g1| + 2|g2| + 2|g3|
+ |g4|)_b`` -- the weight the GPU gate puts on the backward's per-sample d(x) tolerance (Cauchy-Schwarz: |eps . (g_gpu - g)| <=
|eps| G_TOL |g|).
"""
from __future__ import annotations

import math
from typing import Dict, List, NamedTuple, Optional

import torch

from oracle import flow_oracle as fo


class Stage(NamedTuple):
    interval: int
    x: torch.Tensor          # stage state
    t: torch.Tensor          # stage time (0-d, before the factor 999)
    v: torch.Tensor
    g: torch.Tensor          # (dv/dx)^T eps
    d: torch.Tensor          # [B] fp64


class Result(NamedTuple):
    logp: torch.Tensor       # [B] fp64
    z: torch.Tensor
    a: torch.Tensor          # [B] fp64
    gsum: torch.Tensor       # [B] fp64
    stages: List[Stage]


def reversed_grid(n_steps: int, dtype) -> torch.Tensor:
    return fo.rk4_time_grid(n_steps, dtype).flip(0)


def oracle_model(sd: Dict[str, torch.Tensor]):
    """The oracle U-Net as a callable with the model protocol ``model(x, time, cond=...)``."""
    def model(x, time, cond=None):
        return fo.unet_forward(sd, x, time, cond)
    return model


def stage_eval(sd, x, t, cond, eps, t_scale=999):
    """v = unet(x, 999 t, cond), g = (dv/dx)^T eps, d[b] = sum eps g (fp64)."""
    with torch.enable_grad():
        xr = x.detach().requires_grad_(True)
        t_vec = torch.full((x.shape[0],), float(t), dtype=x.dtype)
        v = fo.unet_forward(sd, xr, t_vec * t_scale, cond)
        g, = torch.autograd.grad(v, xr, eps)
    return v.detach(), g.detach(), (eps.double() * g.double()).flatten(1).sum(dim=1)


def log_likelihood_ref(sd, x, n_steps: int, cond: Optional[dict], eps: torch.Tensor) -> Result:
    dtype = x.dtype
    ts = reversed_grid(n_steps, dtype)
    eps = eps.to(dtype)
    a = torch.zeros(x.shape[0], dtype=torch.float64)
    gsum = torch.zeros(x.shape[0], dtype=torch.float64)
    stages: List[Stage] = []
    x = x.detach()
    for i in range(len(ts) - 1):
        t, dt = ts[i], ts[i + 1] - ts[i]
        th = t + dt / 2
        ks, ds, gn = [], [], []
        for xj, tj in ((None, t), (0, th), (1, th), (2, t + dt)):
            xs = x if xj is None else (x + dt * ks[xj] if xj == 2 else x + dt * ks[xj] / 2)
            v, g, d = stage_eval(sd, xs, tj, cond, eps)
            stages.append(Stage(i, xs, tj, v, g, d))
            ks.append(v); ds.append(d); gn.append(g.double().flatten(1).norm(dim=1))
        x = x + (dt / 6) * (ks[0] + 2 * ks[1] + 2 * ks[2] + ks[3])
        a = a + (dt.double() / 6) * (ds[0] + 2 * ds[1] + 2 * ds[2] + ds[3])
        gsum = gsum + (dt.double().abs() / 6) * (gn[0] + 2 * gn[1] + 2 * gn[2] + gn[3])
    D = x[0].numel()
    logp = -0.5 * x.double().flatten(1).pow(2).sum(dim=1) - 0.5 * D * math.log(2 * math.pi) + a
    return Result(logp, x, a, gsum, stages)


def invert_ref(sd, x, n_steps: int, cond: Optional[dict]) -> torch.Tensor:
    """Reversed RK4 without the divergence: data (t = 1) -> noise (t = 0)."""
    ts = reversed_grid(n_steps, x.dtype)
    f = lambda yy, tt: fo.velocity_cfg(sd, cond, 0.0, yy, tt)
    with torch.no_grad():
        for i in range(len(ts) - 1):
            x = fo.rk4_step(f, x, ts[i], ts[i + 1] - ts[i])
    return x


def forward_ref(sd, z, n_steps: int, cond: Optional[dict]) -> torch.Tensor:
    """The oracle's forward RK4 sampler without guidance: noise -> data."""
    with torch.no_grad():
        return fo.generate_latents_rk4(sd, z, n_steps, cond, cfg_strength=0.0)[0]


def a_bound(res: Result, eps: torch.Tensor, g_tol: float) -> torch.Tensor:
    """[B]: g_tol |eps_b| sum_intervals (|dt|/6)(|g1| + 2|g2| + 2|g3| + |g4|)_b."""
    return g_tol * eps.double().flatten(1).norm(dim=1) * res.gsum
