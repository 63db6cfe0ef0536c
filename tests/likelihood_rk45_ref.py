"""Restatement of the adaptive (RK45) flow log-likelihood over the oracle U-Net (test helper, imported by
tests/test_likelihood_rk45_cpu.py, tests/test_gpu_likelihood_rk45.py and tools/make_ll_rk45_golden.py; not a conftest).

scipy's ``RK45`` (the solver ``solve_ivp(method="RK45")`` steps) around ``likelihood_ref.stage_eval``, in the dtype of the state dict
(fp64 for the yardstick), on the concatenated state of one controller group

    y = [x (m unknowns), a (spg unknowns)]        dy/dt = [v(x, 999 t, cond), d]        d[b] = sum_i eps[b,i] ((dv/dx)^T eps)[b,i]

from t0 (a = 0) to t1 < t0.  ``per_sample=False``: one group over the batch (spg = B, m = B*C*H*W); ``per_sample=True``: every sample
its own group (spg = 1, m = C*H*W), the U-Net called on that sample alone with its class id and mask row.  The solver object is stepped
by hand exactly as solve_ivp's loop does (``solver.step()`` until it finishes), so that the evaluations of every ACCEPTED step can be
told apart: besides ``z, a, logp`` and the counters ``[nfev, accepted, rejected]`` per group the result holds

    gsum[b] = sum over accepted steps of |h| sum_s |B_s| |g_s|_b        (B = the fifth-order weights, g_s = (dv/dx)^T eps of stage s)

-- the weight the GPU gate puts on the backward's per-sample d(x) tolerance (Cauchy-Schwarz: |eps . (g_gpu - g)| <= |eps| G_TOL |g|) --
and per group ``margin``, the smallest |error norm - 1| over all its attempts: the distance of its closest accept / reject decision
from going the other way.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

import likelihood_ref as lr


class Rk45Result(NamedTuple):
    logp: torch.Tensor       # [B] fp64
    z: torch.Tensor          # like x
    a: torch.Tensor          # [B] fp64
    counts: np.ndarray       # [G, 3] int64: nfev, accepted, rejected per group
    gsum: torch.Tensor       # [B] fp64
    margin: np.ndarray       # [G] fp64: min over the group's attempts of |error norm - 1|, how far its closest decision was from flipping


def sample_cond(cond: Optional[dict], b: int) -> Optional[dict]:
    return None if not cond else {k: (v[b:b + 1] if torch.is_tensor(v) else v) for k, v in cond.items()}


def augmented_field(sd, shape, cond, eps, record=None):
    """f(t, y) of solve_ivp on y = [x.flatten(), a]; ``record`` (a list) receives |g|_b ([B] fp64) of every evaluation."""
    bsz = shape[0]
    n = int(np.prod(shape))

    def f(t, y):
        x = torch.from_numpy(np.ascontiguousarray(y[:n]).reshape(shape)).to(eps.dtype)
        v, g, d = lr.stage_eval(sd, x, t, cond, eps)
        if record is not None:
            record.append(g.double().flatten(1).norm(dim=1))
        return np.concatenate([v.double().numpy().reshape(-1), d.numpy()])

    return f, np.concatenate([np.zeros(n), np.zeros(bsz)])


def solve_group(sd, x, cond, eps, t0=1.0, t1=0.0, rtol=1e-5, atol=1e-5):
    """One controller group: (z like x, a [spg] fp64, [nfev, accepted, rejected], gsum [spg] fp64, margin)."""
    from scipy.integrate import RK45
    shape, n = tuple(x.shape), x.numel()
    gn = []
    f, y0 = augmented_field(sd, shape, cond, eps, gn)
    y0[:n] = x.double().numpy().reshape(-1)
    solver = RK45(f, t0, y0, t1, rtol=rtol, atol=atol)       # evaluates f(t0, y0): gn[0]
    B5 = np.abs(np.asarray(solver.B, dtype=np.float64))
    gsum = torch.zeros(shape[0], dtype=torch.float64)
    k0, accepted, errs = gn[0], 0, []
    estimate = solver._estimate_error_norm

    def watched(K, h, scale):                                # the error norm of every attempt, as the controller sees it
        errs.append(float(estimate(K, h, scale)))
        return errs[-1]

    solver._estimate_error_norm = watched
    while solver.status == "running":
        msg = solver.step()
        assert solver.status != "failed", msg
        stage = [k0] + gn[-6:-1]                             # K0 (FSAL) and K1..K5 of the accepted attempt; gn[-1] is K6
        gsum += abs(solver.t - solver.t_old) * sum(w * s for w, s in zip(B5, stage))
        k0 = gn[-1]
        accepted += 1
    nfev = int(solver.nfev)
    z = torch.from_numpy(solver.y[:n].reshape(shape).copy()).to(x.dtype)
    margin = float(np.abs(np.array(errs) - 1.0).min())
    return z, torch.from_numpy(solver.y[n:].copy()), [nfev, accepted, (nfev - 2) // 6 - accepted], gsum, margin


def log_likelihood_rk45_ref(sd, x, cond, eps, per_sample=True, t0=1.0, t1=0.0, rtol=1e-5, atol=1e-5) -> Rk45Result:
    eps = eps.to(x.dtype)
    if per_sample:
        parts = [solve_group(sd, x[b:b + 1], sample_cond(cond, b), eps[b:b + 1], t0, t1, rtol, atol) for b in range(x.shape[0])]
        z, a, gsum = (torch.cat([p[i] for p in parts]) for i in (0, 1, 3))
        counts, margin = np.array([p[2] for p in parts], dtype=np.int64), np.array([p[4] for p in parts])
    else:
        z, a, c, gsum, mg = solve_group(sd, x, cond, eps, t0, t1, rtol, atol)
        counts, margin = np.array([c], dtype=np.int64), np.array([mg])
    D = x[0].numel()
    logp = -0.5 * z.double().flatten(1).pow(2).sum(dim=1) - 0.5 * D * math.log(2 * math.pi) + a
    return Rk45Result(logp, z, a, counts, gsum, margin)


# ---- the fixture cases (tools/make_ll_rk45_golden.py writes them, tests/test_gpu_likelihood_rk45.py reads them) ------------------
# At rtol = atol = 1e-5 the solves below carry a global error of 5e-4 .. 1e-2 in z (the two modes of one case differ by that much), and
# how much of it shows between two evaluations of the SAME problem depends on how closely their step sequences agree.  Measured on the
# oracle alone -- the restatement over the fp32 oracle (state fp64, every evaluation on float32(x), float32(t) * 999, as the device
# evaluates) against the fp64 one, 70 candidate cases: z agrees to 1e-7 .. 3e-3 relative, median about 1e-4, with or without equal
# counters, and the distance of the closest accept / reject decision from flipping (``margin``) does not predict it.  The trajectory gate
# of the GPU test (2e-4) is inside that spread, so a fixture is admitted by the reference's own sensitivity to fp32 evaluation: every
# solve of the case (both modes, every sample) must agree between the fp32 and the fp64 oracle to FP32_AGREEMENT = a quarter of the gate
# (the device is another fp32 implementation of the same evaluation), with equal counters, and must contain rejected steps.  The golden
# stores the figure (``z32_rel``) and tests/test_likelihood_rk45_cpu.py asserts it.  Cases are picked by the seed of x.
FP32_AGREEMENT = 5e-5
# id: (Unet kwargs, weight seed, factor on final_conv, B, H = W, name and seed of x, conditioning)
CASES = {
    "d16c10-class": (dict(dim=16, n_classes=10), 5, 0.5, 2, 16, ("llrk45.x.t", 19), [5, 8]),     # the plan with bottleneck attention at n = 4
    "d8mask": (dict(dim=8, n_classes=0, mask_cond=True), 3, 1.0, 2, 8, ("llrk45.x.d8", 5), "mask"),   # the per-sample whole-network plan, mask path
}
RTOL = ATOL = 1e-5


def case_inputs(cid):
    """(state dict, x, eps, cond) of a case from names and seeds alone.  Weights: tools/make_rk45_golden.py's rk45_case_weights (default
    initialisation under the seed, every 1-D parameter + 0.1 randn), final_conv scaled by the case's factor."""
    from oracle.synth import synth_input
    from tools.make_rk45_golden import rk45_case_weights
    kw, seed, fscale, bsz, hw, (xname, xseed), kind = CASES[cid]
    sd = rk45_case_weights(kw, seed)
    for k in ("final_conv.weight", "final_conv.bias"):
        sd[k] = sd[k] * fscale
    x = synth_input(xname, (bsz, 4, hw, hw), xseed)
    eps = torch.where(synth_input("e", (bsz, 4, hw, hw), 1) >= 0, 1.0, -1.0)
    if kind == "mask":
        cond = {"mask_cond": (torch.rand(bsz, 4, hw, hw, generator=torch.Generator().manual_seed(4503)) > 0.35).float()}
    else:
        cond = {"class_cond": torch.tensor(kind)}
    return sd, x, eps, cond
