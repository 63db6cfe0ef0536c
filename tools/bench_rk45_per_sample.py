#!/usr/bin/env python3
"""Per-sample adaptive RK45 at the configuration of tools/bench_rk45.py: flowers-sized U-Net (dim 32, dim_mults [1,2,4,8], 102 classes,
weights seeded as bench.py seeds them), B=64 latents of 4x32x32, class ids, no guidance, AMD_DIRECT_DISPATCH=0.  Prints ONE JSON line
and writes it to --out (default profiles/rk45_per_sample_bench.json):

  batch_forwards              forwards of the whole batch per per-sample solve (= max per-sample nfev)
  nfev_min / median / max     per-sample nfev (each sample its own solve_ivp problem)
  wasted_row_share            share of the evaluated rows that belonged to samples that had already finished (they stay in the batch
                              with h = 0): 1 - sum_b nfev_b / (B * batch_forwards)
  per_sample_ms_per_forward   wall time of a per-sample solve over its batch forwards (median of --reps solves)
  coupled_ms_per_forward      the same for the batch-coupled solve (one step size for the batch), alternating with the per-sample
                              solves in this process; coupled_nfev = its forwards
  ratio_ms_per_forward        per_sample_ms_per_forward / coupled_ms_per_forward
  forwards_vs_coupled         batch_forwards / coupled_nfev: whether per-sample control needs more or fewer batch forwards

    python tools/bench_rk45_per_sample.py [--reps 5] [--out PATH]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rk45_per_sample_bench.json"))
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

    def per_sample():
        return S.generate_latents(model, shape, method="rk45_per_sample", cond=cond, cfg_strength=0.0, source=noise)

    def coupled():
        return S.generate_latents(model, shape, method="rk45", cond=cond, cfg_strength=0.0, source=noise)

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out

    per_sample(); coupled()                                  # warm: plans, graphs, code objects
    tps, tc = [], []
    lat = fwd = nfev_c = None
    for _ in range(a.reps):
        dt, (lat, fwd) = timed(per_sample)
        tps.append(dt)
        dt, (_, nfev_c) = timed(coupled)
        tc.append(dt)
    x = noise.contiguous().clone()
    nfev, acc, rej = model.integrate_rk45(x, 1e-3, 1.0, rtol=1e-5, atol=1e-5, class_ids=ids, per_sample=True)
    assert torch.equal(x, lat) and torch.isfinite(lat).all() and int(nfev.max()) == fwd
    nf = sorted(int(v) for v in nfev)
    rec = {"tool": "bench_rk45_per_sample", "device": torch.cuda.get_device_name(dev), "batch": BATCH, "latent": list(LATENT), "dim": DIM,
           "n_classes": NCLS, "rtol": 1e-5, "atol": 1e-5, "reps": a.reps, "AMD_DIRECT_DISPATCH": os.environ.get("AMD_DIRECT_DISPATCH"),
           "batch_forwards": fwd, "nfev_min": nf[0], "nfev_median": statistics.median(nf), "nfev_max": nf[-1],
           "accepted_total": int(acc.sum()), "rejected_total": int(rej.sum()),
           "wasted_row_share": round(1.0 - sum(nf) / (BATCH * fwd), 4),
           "per_sample_ms_per_solve": round(statistics.median(tps) * 1e3, 2),
           "per_sample_ms_per_forward": round(statistics.median(tps) * 1e3 / fwd, 4),
           "per_sample_spread_ms": [round(min(tps) * 1e3, 2), round(max(tps) * 1e3, 2)],
           "coupled_nfev": nfev_c,
           "coupled_ms_per_solve": round(statistics.median(tc) * 1e3, 2),
           "coupled_ms_per_forward": round(statistics.median(tc) * 1e3 / nfev_c, 4),
           "coupled_spread_ms": [round(min(tc) * 1e3, 2), round(max(tc) * 1e3, 2)]}
    rec["ratio_ms_per_forward"] = round(rec["per_sample_ms_per_forward"] / rec["coupled_ms_per_forward"], 4)
    rec["forwards_vs_coupled"] = round(fwd / nfev_c, 4)
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
