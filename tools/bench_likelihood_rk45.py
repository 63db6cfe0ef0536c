#!/usr/bin/env python3
"""The adaptive (RK45) log-likelihood against the RK4 likelihood at the configuration of tools/bench_rk45.py: flowers-sized U-Net (dim 32,
dim_mults [1,2,4,8], 102 classes, weights seeded as bench.py seeds them), B=64 latents of 4x32x32, class ids, one Rademacher probe.
The two solves alternate in this process, the plans stay in the training form throughout (restore_plan=False).  Prints ONE JSON line
and writes it to --out (default profiles/likelihood_rk45_bench.json):

  rk4_ms_per_eval             Unet.log_likelihood on --rk4-steps grid points: wall time over its 4 (n - 1) evaluations (median of --reps);
                              rk4_spread_ms_per_eval = (min, max) over the repetitions, rk4_spread_rel = (max - min) / median
  rk45_ms_per_eval            Unet.log_likelihood_rk45 (rtol = atol = 1e-5) over its batch evaluations (per sample: the largest nfev), for
                              both modes, with nfev / accepted / rejected (per sample: min / median / max and totals)
  expectation                 per evaluation the adaptive solve should cost no more than the RK4 likelihood times what the RK45 sampler costs
                              over the RK4 sampler per evaluation (SAMPLER_RATIO, 1.02 on record), within the spread this tool measures on
                              the RK4 likelihood itself: rk45 <= rk4 * SAMPLER_RATIO * (1 + rk4_spread_rel).  Reported as met / missed per
                              mode, never asserted
  logp_abs_diff_vs_rk4        |logp_rk45 - logp_rk4(n_steps)| for n_steps = 10, 50, 200 against the per-sample adaptive solve: max and
                              median over the batch, also in bits per dimension -- what the fixed grid was costing

    python tools/bench_likelihood_rk45.py [--reps 3] [--out PATH]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if not os.environ.get("FLOCODER_AMD_KEEP_ENV"):
    os.environ.setdefault("AMD_DIRECT_DISPATCH", "0")      # the sampler's shipping runtime mode, as bench.py

import torch  # noqa: E402

BATCH, LATENT, DIM, NCLS = 64, (4, 32, 32), 32, 102
SAMPLER_RATIO = 1.02                                       # RK45 sampler over RK4 sampler, ms per evaluation (profiles/rk45_bench.json era)
GRIDS = (10, 50, 200)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rk4-steps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "likelihood_rk45_bench.json"))
    a = ap.parse_args()
    from flocoder_amd import sampling as S
    from flocoder_amd.unet import Unet
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = Unet(dim=DIM, dim_mults=(1, 2, 4, 8), channels=LATENT[0], n_classes=NCLS).eval().to(dev)
    g = torch.Generator().manual_seed(1234)
    x0 = torch.randn((BATCH,) + LATENT, generator=g).to(dev)
    eps = (torch.randint(0, 2, (BATCH,) + LATENT, generator=g).float() * 2 - 1).to(dev)
    ids = torch.randint(NCLS, (BATCH,), generator=torch.Generator().manual_seed(1235)).to(dev)

    def rk4(n):
        x = x0.clone()
        _, logp = model.log_likelihood(x, S.rk4_time_grid(n).flip(0), eps, class_ids=ids, restore_plan=False)
        return logp, 4 * (n - 1)

    def rk45(per_sample):
        x = x0.clone()
        (nfev, acc, rej), _, logp = model.log_likelihood_rk45(x, eps, per_sample=per_sample, class_ids=ids, restore_plan=False)
        return logp, (nfev, acc, rej)

    def timed(fn, *args):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn(*args)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out

    rk4(3); rk45(True); rk45(False)                          # warm: plans, code objects
    t4, tp, tc = [], [], []
    for _ in range(a.reps):
        dt, (_, evals4) = timed(rk4, a.rk4_steps)
        t4.append(dt * 1e3 / evals4)
        dt, (logp_ps, cps) = timed(rk45, True)
        tp.append(dt * 1e3 / int(cps[0].max()))
        dt, (logp_c, cc) = timed(rk45, False)
        tc.append(dt * 1e3 / cc[0])
    m4 = statistics.median(t4)
    spread = (max(t4) - min(t4)) / m4
    limit = m4 * SAMPLER_RATIO * (1 + spread)
    nf = sorted(int(v) for v in cps[0])
    D = math.prod(LATENT)
    diffs = {}
    for n in GRIDS:
        d = (logp_ps - rk4(n)[0]).abs()
        diffs[str(n)] = {"max": float(d.max()), "median": float(d.median()), "max_bits_per_dim": float(d.max()) / (D * math.log(2.0))}
    model.release_training_plan()
    rec = {"tool": "bench_likelihood_rk45", "device": torch.cuda.get_device_name(dev), "batch": BATCH, "latent": list(LATENT), "dim": DIM,
           "n_classes": NCLS, "rtol": 1e-5, "atol": 1e-5, "reps": a.reps, "AMD_DIRECT_DISPATCH": os.environ.get("AMD_DIRECT_DISPATCH"),
           "rk4_steps": a.rk4_steps, "rk4_ms_per_eval": round(m4, 4), "rk4_spread_ms_per_eval": [round(min(t4), 4), round(max(t4), 4)],
           "rk4_spread_rel": round(spread, 4), "sampler_ratio": SAMPLER_RATIO, "limit_ms_per_eval": round(limit, 4),
           "per_sample": {"ms_per_eval": round(statistics.median(tp), 4), "spread_ms_per_eval": [round(min(tp), 4), round(max(tp), 4)],
                          "batch_evaluations": nf[-1], "nfev_min": nf[0], "nfev_median": statistics.median(nf), "nfev_max": nf[-1],
                          "accepted_total": int(cps[1].sum()), "rejected_total": int(cps[2].sum())},
           "coupled": {"ms_per_eval": round(statistics.median(tc), 4), "spread_ms_per_eval": [round(min(tc), 4), round(max(tc), 4)],
                       "nfev": cc[0], "accepted": cc[1], "rejected": cc[2]},
           "logp_abs_diff_vs_rk4": diffs,
           "logp_abs_diff_coupled_vs_per_sample": float((logp_c - logp_ps).abs().max())}
    for mode in ("per_sample", "coupled"):
        rec[mode]["ratio_vs_rk4"] = round(rec[mode]["ms_per_eval"] / m4, 4)
        rec[mode]["expectation"] = "met" if rec[mode]["ms_per_eval"] <= limit else "missed"
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
