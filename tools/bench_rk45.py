#!/usr/bin/env python3
"""Adaptive RK45 sampler at the headline's model and batch: flowers-sized U-Net (dim 32, dim_mults [1,2,4,8], 102 classes, weights
seeded as bench.py seeds them), B=64 latents of 4x32x32, class ids, no guidance.  Prints ONE JSON line:

  nfev / accepted / rejected   scipy's counters of the device solve (Unet.integrate_rk45 via sampling.generate_latents_rk45)
  rk45_ms_per_eval             wall time of a whole solve over its nfev (median of --reps solves)
  rk4_ms_per_eval              the fixed-grid RK4 integrator (--rk4-steps grid points) on the same model and batch, over its evaluations,
                               alternating with the RK45 solves in this process
  ratio                        rk45_ms_per_eval / rk4_ms_per_eval
  legacy_ms_per_eval           the legacy path for scale (legacy/train_sd_flowers.py:78-107): scipy solve_ivp on the host calling
                               model.forward through numpy copies, one solve

    python tools/bench_rk45.py [--reps 5] [--rk4-steps 26] [--no-legacy]

With ``--t-eval N [N ...]`` (e.g. ``--t-eval 8 64``) it measures dense output instead: the same solve with 0 and with N evenly spaced
requested times over [1e-3, 1], alternating in this process, and prints ONE JSON line with the per-solve medians, their spreads and the
ratios against 0 times (profiles/rk45_dense_bench.json), after checking that the latents and nfev do not depend on t_eval.
"""
import argparse
import json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rk4-steps", type=int, default=26)
    ap.add_argument("--no-legacy", action="store_true")
    ap.add_argument("--t-eval", type=int, nargs="+", metavar="N", help="time dense output with 0 and N requested times instead")
    a = ap.parse_args()
    from flocoder_amd import sampling as S
    from flocoder_amd.unet import Unet
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = Unet(dim=DIM, dim_mults=(1, 2, 4, 8), channels=LATENT[0], n_classes=NCLS).eval().to(dev)
    noise = torch.randn((BATCH,) + LATENT, generator=torch.Generator().manual_seed(1234)).to(dev)
    ids = torch.randint(NCLS, (BATCH,), generator=torch.Generator().manual_seed(1235)).to(dev)
    shape = (BATCH,) + LATENT
    cond = {"class_cond": ids}

    def rk45():
        return S.generate_latents_rk45(model, shape, cond=cond, cfg_strength=0.0, source=noise)

    def rk4():
        return S.generate_latents_rk4(model, shape, a.rk4_steps, cond, 0.0, source=noise)

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out

    if a.t_eval:
        counts = [0] + [n for n in a.t_eval if n > 0]
        times = {n: (torch.linspace(1e-3, 1.0, n, dtype=torch.float64).tolist() if n else None) for n in counts}

        def dense(n):
            return S.generate_latents_rk45(model, shape, cond=cond, cfg_strength=0.0, source=noise, t_eval=times[n])

        ref = None
        for n in counts:                                     # warm both graph shapes; t_eval must not change the solve
            out = dense(n)
            ref = ref or out
            assert torch.equal(out[0], ref[0]) and out[1] == ref[1] and (n == 0 or torch.isfinite(out[2]).all())
        ts = {n: [] for n in counts}
        for _ in range(a.reps):
            for n in counts:
                ts[n].append(timed(lambda: dense(n))[0])
        med = {n: statistics.median(v) * 1e3 for n, v in ts.items()}
        rec = {"tool": "bench_rk45 --t-eval", "device": torch.cuda.get_device_name(dev), "batch": BATCH, "latent": list(LATENT), "dim": DIM,
               "n_classes": NCLS, "rtol": 1e-5, "atol": 1e-5, "reps": a.reps, "AMD_DIRECT_DISPATCH": os.environ.get("AMD_DIRECT_DISPATCH"),
               "nfev": ref[1], "t_eval_counts": counts,
               "ms_per_solve": {str(n): round(med[n], 2) for n in counts},
               "spread_ms": {str(n): [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)] for n, v in ts.items()},
               "ratio_to_0": {str(n): round(med[n] / med[0], 4) for n in counts if n},
               "frame_mbytes": {str(n): round(n * BATCH * LATENT[0] * LATENT[1] * LATENT[2] * 4 / 1e6, 2) for n in counts if n}}
        print(json.dumps(rec), flush=True)
        return

    rk45(); rk4()                                            # warm: plans, graphs, code objects
    t45, t4 = [], []
    lat = nfev = None
    for _ in range(a.reps):
        dt, (lat, nfev) = timed(rk45)
        t45.append(dt)
        dt, _ = timed(rk4)
        t4.append(dt)
    x = noise.contiguous().clone()
    _, acc, rej = model.integrate_rk45(x, 1e-3, 1.0, rtol=1e-5, atol=1e-5, class_ids=ids)
    assert torch.equal(x, lat) and torch.isfinite(lat).all()
    rk4_evals = (a.rk4_steps - 1) * 4
    rec = {"tool": "bench_rk45", "device": torch.cuda.get_device_name(dev), "batch": BATCH, "latent": list(LATENT), "dim": DIM,
           "n_classes": NCLS, "rtol": 1e-5, "atol": 1e-5, "reps": a.reps,
           "AMD_DIRECT_DISPATCH": os.environ.get("AMD_DIRECT_DISPATCH"),
           "nfev": nfev, "accepted": acc, "rejected": rej,
           "rk45_ms_per_solve": round(statistics.median(t45) * 1e3, 2),
           "rk45_ms_per_eval": round(statistics.median(t45) * 1e3 / nfev, 4),
           "rk4_evals": rk4_evals, "rk4_ms_per_eval": round(statistics.median(t4) * 1e3 / rk4_evals, 4),
           "rk45_spread_ms": [round(min(t45) * 1e3, 2), round(max(t45) * 1e3, 2)],
           "rk4_spread_ms": [round(min(t4) * 1e3, 2), round(max(t4) * 1e3, 2)]}
    rec["ratio"] = round(rec["rk45_ms_per_eval"] / rec["rk4_ms_per_eval"], 4)
    if not a.no_legacy:
        class HostPath(torch.nn.Module):      # not a flocoder_amd.Unet: rk45_sampler takes the legacy scipy path through numpy
            def __init__(self, m):
                super().__init__()
                self.m = m

            def forward(self, x, t, cond=None):
                return self.m(x, t, cond)

        dt, (ref, nfev_l) = timed(lambda: S.rk45_sampler(HostPath(model), shape, device=dev, cond=cond, source=noise))
        d = (ref.double() - lat.double()).norm() / ref.double().norm()
        rec.update({"legacy_nfev": nfev_l, "legacy_ms_per_eval": round(dt * 1e3 / nfev_l, 4), "legacy_s": round(dt, 2),
                    "device_vs_legacy_rel_l2": float(d)})
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
