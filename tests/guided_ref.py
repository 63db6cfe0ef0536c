"""Restatement of measurement-guided RK4 sampling (flocoder_amd.sampling.generate_latents_guided) over the oracle U-Net or any callable
field (test helper, imported by tests/test_guided_cpu.py and tests/test_gpu_guided.py; not a conftest).

Written from the formulas of DESIGN.md section 4, not from the code under test, in the dtype of the inputs (fp64 for the yardstick).  With
``y`` the measurement, ``a`` the keep weights, and for every RK4 stage its own input state x and time t:

    x1 = x + (1-t) v     r2 = (1-t)^2 / (t^2 + (1-t)^2)     w = a (y - a x1) / (r2 a^2 + sigma_y^2)   (0 where the denominator is 0)
    g  = w  (identity)   |   w + (1-t) (dv/dx)^T w  (exact)                     v_c = v + gamma ((1-t)/t) g

``v`` is the oracle's velocity after classifier-free guidance (``flow_oracle.velocity_cfg``); the exact form differentiates the plain
forward and takes no guidance.  The start is ``(1 - s) source + s init_latents`` and the grid ``rk4_time_grid(n_steps, s)``, as
``flow_oracle.generate_latents_rk4`` with ``init_latents``.
"""
from __future__ import annotations

from typing import Callable, List, NamedTuple, Optional

import torch

from oracle import flow_oracle as fo


class Stage(NamedTuple):
    interval: int
    x: torch.Tensor          # stage state
    t: torch.Tensor          # stage time (0-d, before the factor 999)
    v: torch.Tensor          # velocity before the correction
    w: torch.Tensor
    q: Optional[torch.Tensor]    # (dv/dx)^T w, exact form only
    vc: torch.Tensor         # corrected velocity


class Result(NamedTuple):
    latents: torch.Tensor
    start: torch.Tensor
    ts: torch.Tensor
    stages: List[Stage]


def weight(v, x, t, y, a, sigma_y):
    """w of the formulas above; 0 where r2 a^2 + sigma_y^2 = 0."""
    om = 1 - t
    x1 = x + om * v
    r2 = om * om / (t * t + om * om)
    den = r2 * a * a + sigma_y * sigma_y
    num = a * (y - a * x1)
    safe = torch.where(den == 0, torch.ones_like(den), den)
    return torch.where(den == 0, torch.zeros_like(num), num / safe)


def correct(v, x, t, y, a, sigma_y, gamma, q=None):
    """v_c; ``q`` = (dv/dx)^T w for the exact form."""
    om = 1 - t
    w = weight(v, x, t, y, a, sigma_y)
    g = w if q is None else w + om * q
    return v + gamma * (om / t) * g


def field_stage(field: Callable, x, t, y, a, sigma_y, gamma, exact: bool):
    """One corrected evaluation of ``field(x, t) -> v`` (differentiable in x for the exact form) -> (v, w, q, v_c)."""
    if not exact:
        with torch.no_grad():
            v = field(x, t)
        w = weight(v, x, t, y, a, sigma_y)
        return v, w, None, correct(v, x, t, y, a, sigma_y, gamma)
    with torch.enable_grad():
        xr = x.detach().requires_grad_(True)
        vr = field(xr, t)
        v = vr.detach()
        w = weight(v, x, t, y, a, sigma_y)
        q, = torch.autograd.grad(vr, xr, w)
    return v, w, q.detach(), correct(v, x, t, y, a, sigma_y, gamma, q.detach())


def guided_rk4(field: Callable, start, ts, y, a, sigma_y, gamma, exact: bool) -> Result:
    """The classic RK4 step along ``ts`` over the corrected field; every stage recorded."""
    x = start.detach()
    stages: List[Stage] = []
    for i in range(len(ts) - 1):
        t, dt = ts[i], ts[i + 1] - ts[i]
        th = t + dt / 2
        ks = []
        for xj, tj in ((None, t), (0, th), (1, th), (2, t + dt)):
            xs = x if xj is None else (x + dt * ks[xj] if xj == 2 else x + dt * ks[xj] / 2)
            v, w, q, vc = field_stage(field, xs, tj, y, a, sigma_y, gamma, exact)
            stages.append(Stage(i, xs, tj, v, w, q, vc))
            ks.append(vc)
        x = x + (dt / 6) * (ks[0] + 2 * ks[1] + 2 * ks[2] + ks[3])
    return Result(x, start, ts, stages)


def oracle_field(sd, cond, cfg_strength, t_scale=999):
    """The oracle U-Net as ``field(x, t)``: sampling.py's v_func with guidance (differentiable when ``cfg_strength`` is 0)."""
    def field(x, t):
        if cfg_strength and cond and cond.get("class_cond") is not None:
            return fo.velocity_cfg(sd, cond, cfg_strength, x, t)
        t_vec = torch.full((x.shape[0],), float(t), dtype=x.dtype)
        return fo.unet_forward(sd, x, t_vec * t_scale, cond)
    return field


def guided_ref(sd, source, measurement, keep, n_steps: int, init_strength: float, cond: Optional[dict], cfg_strength: float,
               sigma_y: float, gamma: float, jacobian: str = "identity", init_latents=None) -> Result:
    """generate_latents_guided over the oracle U-Net with state dict ``sd``, in the dtype of ``source``."""
    dtype = source.dtype
    y, a = measurement.to(dtype), keep.to(dtype)
    init = y if init_latents is None else init_latents.to(dtype)
    start = (1 - init_strength) * source + init_strength * init
    ts = fo.rk4_time_grid(n_steps, dtype, init_strength=init_strength)
    if jacobian == "exact":
        assert not (cfg_strength and cond and cond.get("class_cond") is not None), "the exact form takes no guidance"
    return guided_rk4(oracle_field(sd, cond, cfg_strength), start, ts, y, a, sigma_y, gamma, jacobian == "exact")


def unguided_ref(sd, source, measurement, n_steps, init_strength, cond, cfg_strength, init_latents=None) -> torch.Tensor:
    """The same start through the oracle's plain sampler."""
    init = measurement if init_latents is None else init_latents
    with torch.no_grad():
        return fo.generate_latents_rk4(sd, source, n_steps, cond, cfg_strength, init_latents=init.to(source.dtype), init_strength=init_strength)[0]


def kept_residual(x1, keep, known) -> torch.Tensor:
    """[B]: | keep (x1 - known) | per sample."""
    return (keep.double() * (x1.double() - known.double())).flatten(1).norm(dim=1)


# ------------------------------------------------------------------------------------------- the GPU test's cases
# The likelihood test's models (tests/test_gpu_likelihood.py): id -> (shape table, seed, B, H = W, conditioning, cfg_strength, n_steps).
# init_strength 0.2, sigma_y 0.05, gamma 1 throughout: the defaults of generate_latents_guided.
CASES = {
    "d16c10-class-cfg3": ("d16c10", 2, 3, 16, "class", 3.0, 10),
    "d16c10-nocond": ("d16c10", 2, 3, 16, None, 0.0, 10),
    "d32c102-class": ("d32c102", 1, 2, 32, "class", 0.0, 6),
    "d8mask": ("d8mask", 3, 3, 8, "mask", 0.0, 10),
}
INIT_STRENGTH, SIGMA_Y, GAMMA = 0.2, 0.05, 1.0


def case_inputs(cid):
    """-> dict(sd, source, known, keep, measurement, cond, cfg, n): fp32 CPU tensors; keep is a 0/1 mask [B,1,H,W] that measures about
    60 % of the pixels (all four channels of a pixel together), measurement = keep * known."""
    from conftest import load_golden
    from oracle.synth import synth_input, synth_state_dict
    tag, seed, bsz, hw, kind, cfg, n = CASES[cid]
    sd = synth_state_dict(load_golden("g3_unet_" + tag)["shapes"], seed)
    meta = fo.unet_meta(sd)
    g = torch.Generator().manual_seed(4000 + seed)
    source = synth_input(f"guided.src.{cid}", (bsz, 4, hw, hw), seed)
    known = synth_input(f"guided.known.{cid}", (bsz, 4, hw, hw), seed)
    keep = (torch.rand(bsz, 1, hw, hw, generator=g) > 0.4).float()
    cond = {}
    if kind == "class":
        cond["class_cond"] = torch.randint(0, meta["n_classes"], (bsz,), generator=g)
    elif kind == "mask":
        cond["mask_cond"] = (torch.rand(bsz, 4, hw, hw, generator=g) > 0.35).float()
    return dict(sd=sd, source=source, known=known, keep=keep, measurement=keep * known, cond=cond or None, cfg=cfg, n=n)


def case_refs(cid, which=("identity", "exact", "unguided")):
    """The fp64 restatement of a case -> {"identity": Result at the case's cfg_strength, "exact": Result without guidance,
    "unguided": latents of the plain sampler at the case's cfg_strength, "identity0": Result without guidance}."""
    c = case_inputs(cid)
    sd64 = {k: v.double() for k, v in c["sd"].items()}
    src, y, a = c["source"].double(), c["measurement"].double(), c["keep"].double()
    out = {}
    for w in which:
        if w == "unguided":
            out[w] = unguided_ref(sd64, src, y, c["n"], INIT_STRENGTH, c["cond"], c["cfg"])
        else:
            cfg = c["cfg"] if w == "identity" else 0.0
            out[w] = guided_ref(sd64, src, y, a, c["n"], INIT_STRENGTH, c["cond"], cfg, SIGMA_Y, GAMMA, "exact" if w == "exact" else "identity")
    return out
