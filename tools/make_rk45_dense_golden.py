#!/usr/bin/env python3
"""tests/golden/rk45_dense_scipy_oracle.npz: the adaptive sampler's trajectory at requested times.  The same solves as
tools/make_rk45_golden.py (batch-coupled) and tools/make_rk45_per_sample_golden.py (one solve per sample) -- scipy.integrate.solve_ivp(
method="RK45", rtol = atol = 1e-5) over (1e-3, 1) around the CPU oracle U-Net -- with ``t_eval = T_EVAL``: every accepted step evaluates
its quartic interpolant (scipy's RkDenseOutput) at the requested times inside it.  The cases, weights and sources are those tools'
(imported, not restated); their own fixtures are not touched.  Each case stores its source, t_eval, the frames ([F, B, C, H, W], fp32)
and the final latents and [nfev, accepted, rejected] of the SAME solve (the last requested time is t1, but the final latents are the
solver's own y(t1), taken from a recording of its accepted steps, not the interpolant there).

Keys: "coupled.<case>.*" and "per_sample.<case>.*"; per-sample counts are [B, 3].

    python tools/make_rk45_dense_golden.py        (minutes on the host: hundreds of oracle forwards per solve)
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import flow_oracle as fo  # noqa: E402
from tools.make_rk45_golden import ATOL, EPS, RTOL, case_inputs  # noqa: E402
from tools.make_rk45_per_sample_golden import per_sample_inputs, sample_cond  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "rk45_dense_scipy_oracle.npz")
T_EVAL = (1e-3, 0.05, 0.25, 0.5, 0.75, 0.9, 1.0)      # both end points, and several values inside the long late steps
COUPLED = ("d16_cfg3", "d8mask", "d32")
PER_SAMPLE = ("d16_mixed", "d8mask")


@torch.no_grad()
def scipy_oracle_dense(sd, z0, cond, cfg, t_eval=T_EVAL):
    """(frames [F, *shape], latents, nfev, accepted, rejected) of solve_ivp(RK45, t_eval) on velocity_cfg.  With t_eval scipy returns only
    the requested times, so the solver's own final state and its accepted-step count come from a terminal event that never fires:
    solve_ivp evaluates events at every accepted (t, y) and changes nothing else about the steps."""
    from scipy.integrate import solve_ivp
    shape = tuple(z0.shape)
    steps = []

    def f(t, y):
        x = torch.from_numpy(y.reshape(shape)).type(torch.float32)
        return fo.velocity_cfg(sd, cond, cfg, x, t).numpy().reshape(-1)

    def watch(t, y):
        steps.append((float(t), np.array(y, dtype=np.float64)))
        return 1.0

    sol = solve_ivp(f, (EPS, 1), z0.numpy().reshape(-1), method="RK45", rtol=RTOL, atol=ATOL, t_eval=np.asarray(t_eval, dtype=np.float64),
                    events=watch)
    assert sol.success and sol.status == 0, sol.message
    assert sol.y.shape[1] == len(t_eval) and steps[0][0] == EPS and steps[-1][0] == 1.0
    acc = len(steps) - 1                                   # (the first call is the event's value at t0)
    frames = torch.tensor(sol.y.T.copy()).reshape((len(t_eval),) + shape).type(torch.float32)
    lat = torch.tensor(steps[-1][1]).reshape(shape).type(torch.float32)
    return frames, lat, int(sol.nfev), acc, (int(sol.nfev) - 2) // 6 - acc


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    names = sys.argv[1:] or ["coupled." + n for n in COUPLED] + ["per_sample." + n for n in PER_SAMPLE]
    out = dict(np.load(OUT)) if os.path.exists(OUT) else {}
    for key in names:
        mode, name = key.split(".", 1)
        if mode == "coupled":
            sd, z0, cond, cfg = case_inputs(name)
            frames, lat, nfev, acc, rej = scipy_oracle_dense(sd, z0, cond, cfg)
            counts = [nfev, acc, rej]
        else:
            sd, z0, cond, cfg = per_sample_inputs(name)
            per = [scipy_oracle_dense(sd, z0[b:b + 1], sample_cond(cond, b), cfg) for b in range(z0.shape[0])]
            frames, lat = torch.cat([p[0] for p in per], dim=1), torch.cat([p[1] for p in per])
            counts = [list(p[2:]) for p in per]
        out[f"{key}.source"] = z0.numpy()
        out[f"{key}.t_eval"] = np.asarray(T_EVAL, dtype=np.float64)
        out[f"{key}.frames"] = frames.numpy()
        out[f"{key}.latents"] = lat.numpy()
        out[f"{key}.counts"] = np.array(counts, dtype=np.int64)
        print(json.dumps({"case": key, "counts": counts}), flush=True)
        np.savez_compressed(OUT, **out)


if __name__ == "__main__":
    main()
