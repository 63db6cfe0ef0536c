"""Restatement of the K-probe adaptive (RK45) flow log-likelihood over the oracle U-Net (test helper, imported by
tests/test_likelihood_probes_cpu.py, tests/test_gpu_likelihood_probes.py and tools/make_ll_probes_golden.py; not a conftest).

tests/likelihood_rk45_ref.py with K Hutchinson probes eps_1..eps_K in one solve: the state of a controller group stays

    y = [x (m unknowns), a (spg unknowns)]        dy/dt = [v(x, 999 t, cond), dbar]        dbar = (d_1 + ... + d_K) / K

with d_k[b] = sum_i eps_k[b,i] ((dv/dx)^T eps_k)[b,i] of ONE forward (K gradients of the same graph), summed in probe order with one
division.  The solver object is stepped by hand as there, so besides ``z, a, logp``, the counters and ``margin`` the result holds per
probe

    a_probes[k][b] = sum over accepted steps of h sum_s B_s d_{s,k}[b]          (the per-probe integrals: by-products outside the norm)
    gsum[k][b]     = sum over accepted steps of |h| sum_s |B_s| |g_{s,k}|_b      (the weight of the backward's d(x) tolerance, per probe)

The cases are likelihood_rk45_ref's (same models, latents, conditioning, tolerances, first probe) with two more probes from fixed seeds.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

import likelihood_rk45_ref as rr
from oracle import flow_oracle as fo


class ProbesResult(NamedTuple):
    logp: torch.Tensor       # [B] fp64
    z: torch.Tensor          # like x
    a: torch.Tensor          # [B] fp64: the solve's own a (the integral of the mean)
    counts: np.ndarray       # [G, 3] int64: nfev, accepted, rejected per group
    gsum: torch.Tensor       # [K, B] fp64
    margin: np.ndarray       # [G] fp64
    a_probes: torch.Tensor   # [K, B] fp64


def stage_eval_probes(sd, x, t, cond, eps_k, t_scale=999):
    """v = unet(x, 999 t, cond); g_k = (dv/dx)^T eps_k for every probe from the one forward; d_k[b] = sum eps_k g_k (fp64) -> (v, g [K, ...],
    d [K, B])."""
    n_k = eps_k.shape[0]
    with torch.enable_grad():
        xr = x.detach().requires_grad_(True)
        t_vec = torch.full((x.shape[0],), float(t), dtype=x.dtype)
        v = fo.unet_forward(sd, xr, t_vec * t_scale, cond)
        g = torch.stack([torch.autograd.grad(v, xr, eps_k[k], retain_graph=k + 1 < n_k)[0] for k in range(n_k)])
    return v.detach(), g.detach(), (eps_k.double() * g.double()).flatten(2).sum(dim=2)


def mean_in_probe_order(d):
    """(d[0] + d[1] + ... + d[K-1]) / K, left to right, one division"""
    s = d[0]
    for k in range(1, d.shape[0]):
        s = s + d[k]
    return s / d.shape[0]


def solve_group(sd, x, cond, eps_k, t0=1.0, t1=0.0, rtol=1e-5, atol=1e-5):
    """One controller group: (z like x, a [spg], [nfev, accepted, rejected], gsum [K, spg], margin, a_probes [K, spg])."""
    from scipy.integrate import RK45
    shape, n = tuple(x.shape), x.numel()
    gn, dk = [], []                                          # per evaluation: |g_k|_b [K, spg] and d_k [K, spg]

    def f(t, y):
        xx = torch.from_numpy(np.ascontiguousarray(y[:n]).reshape(shape)).to(eps_k.dtype)
        v, g, d = stage_eval_probes(sd, xx, t, cond, eps_k)
        gn.append(g.double().flatten(2).norm(dim=2))
        dk.append(d)
        return np.concatenate([v.double().numpy().reshape(-1), mean_in_probe_order(d).numpy()])

    y0 = np.concatenate([x.double().numpy().reshape(-1), np.zeros(shape[0])])
    solver = RK45(f, t0, y0, t1, rtol=rtol, atol=atol)
    B5 = np.asarray(solver.B, dtype=np.float64)
    gsum = torch.zeros(eps_k.shape[0], shape[0], dtype=torch.float64)
    a_probes = torch.zeros_like(gsum)
    g0, d0, accepted, errs = gn[0], dk[0], 0, []
    estimate = solver._estimate_error_norm

    def watched(K, h, scale):
        errs.append(float(estimate(K, h, scale)))
        return errs[-1]

    solver._estimate_error_norm = watched
    while solver.status == "running":
        msg = solver.step()
        assert solver.status != "failed", msg
        h = solver.t - solver.t_old
        gsum += abs(h) * sum(abs(w) * s for w, s in zip(B5, [g0] + gn[-6:-1]))
        a_probes += h * sum(w * s for w, s in zip(B5, [d0] + dk[-6:-1]))
        g0, d0 = gn[-1], dk[-1]
        accepted += 1
    nfev = int(solver.nfev)
    z = torch.from_numpy(solver.y[:n].reshape(shape).copy()).to(x.dtype)
    margin = float(np.abs(np.array(errs) - 1.0).min())
    return z, torch.from_numpy(solver.y[n:].copy()), [nfev, accepted, (nfev - 2) // 6 - accepted], gsum, margin, a_probes


def log_likelihood_probes_ref(sd, x, cond, eps_k, per_sample=True, t0=1.0, t1=0.0, rtol=1e-5, atol=1e-5) -> ProbesResult:
    eps_k = eps_k.to(x.dtype)
    if per_sample:
        parts = [solve_group(sd, x[b:b + 1], rr.sample_cond(cond, b), eps_k[:, b:b + 1], t0, t1, rtol, atol) for b in range(x.shape[0])]
        z, a = (torch.cat([p[i] for p in parts]) for i in (0, 1))
        gsum, a_probes = (torch.cat([p[i] for p in parts], dim=1) for i in (3, 5))
        counts, margin = np.array([p[2] for p in parts], dtype=np.int64), np.array([p[4] for p in parts])
    else:
        z, a, c, gsum, mg, a_probes = solve_group(sd, x, cond, eps_k, t0, t1, rtol, atol)
        counts, margin = np.array([c], dtype=np.int64), np.array([mg])
    D = x[0].numel()
    logp = -0.5 * z.double().flatten(1).pow(2).sum(dim=1) - 0.5 * D * math.log(2 * math.pi) + a
    return ProbesResult(logp, z, a, counts, gsum, margin, a_probes)


# ---- the fixture cases -----------------------------------------------------------------------------------------------------------------
# likelihood_rk45_ref.CASES with two more probes each: +-1 from the sign of synth_input("llp.e", shape, seed) for the seeds below.  The
# cases are admitted like the single-probe golden's (likelihood_rk45_ref.FP32_AGREEMENT; tools/make_ll_probes_golden.py records which
# seeds were tried).
PROBE_SEEDS = {"d16c10-class": (103, 104), "d8mask": (105, 106)}
N_PROBES = 3


def case_inputs(cid, seeds=None):
    """(state dict, x, eps [3, B, C, H, W], cond): likelihood_rk45_ref.case_inputs with the case's two further probes behind its own."""
    from oracle.synth import synth_input
    sd, x, eps, cond = rr.case_inputs(cid)
    more = [torch.where(synth_input("llp.e", tuple(x.shape), s) >= 0, 1.0, -1.0) for s in (seeds or PROBE_SEEDS[cid])]
    return sd, x, torch.stack([eps] + more), cond
