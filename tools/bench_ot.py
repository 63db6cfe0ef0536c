#!/usr/bin/env python3
"""What the exact mini-batch OT pairing costs and buys, against the greedy matcher: D = 4096 (the stl_sd.yaml latent, 4x32x32),
B = 64, 128, 256, a Gaussian source against a fixed-seed Gaussian target batch (the solver's augmenting-path count depends on the data:
these figures are for that input).

    python tools/bench_ot.py [--batches 64 128 256 --reps 50 --steps 20 --windows 5 --out profiles/ot_exact_bench.json]

Per batch size: the time per call of either pairing alone (windows of --reps calls between device synchronisations, the two methods
alternating, median and spread over the windows), pairing_cost of the identity, greedy and exact pairings (mean over the sources used),
and FlowTrainer.step (U-Net dim 32, the pairing call inside the step) with either method, timed the same way.  The expectation checked
and reported: step(exact) <= step(greedy) + (exact alone - greedy alone) + the run-to-run spread of step(greedy) -- the new path adds
its own kernels' time and no hidden synchronisation or stall."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def windows(fns, n_windows, reps, device):
    """{name: [ms per call, one figure per window]}, the functions alternating window by window."""
    out = {k: [] for k in fns}
    for _ in range(n_windows):
        for name, fn in fns.items():
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for r in range(reps):
                fn(r)
            torch.cuda.synchronize(device)
            out[name].append(1e3 * (time.perf_counter() - t0) / reps)
    return out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "spread_ms": round(max(ms) - min(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--sources", type=int, default=8)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ot_exact_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ot.py measures on an MI355X; no GPU found")
    from flocoder_amd.ot import compute_ot_pairing, pairing_cost
    from flocoder_amd.train import FlowTrainer
    from flocoder_amd.unet import Unet
    device = torch.device("cuda", 0)
    results = []
    for B in args.batches:
        g = torch.Generator().manual_seed(1234 + B)
        target = torch.randn(B, 4, 32, 32, generator=g).to(device)
        sources = [torch.randn(B, 4, 32, 32, generator=g).to(device) for _ in range(args.sources)]
        cls = torch.randint(10, (B,), generator=g).to(device)
        pair = {m: (lambda r, m=m: compute_ot_pairing(sources[r % len(sources)], target, method=m)) for m in ("greedy", "exact")}
        costs = {"identity": [], "greedy": [], "exact": []}
        for s in sources:                                      # also the warm-up of both methods at this shape
            costs["identity"].append(float(pairing_cost(s, target)))
            for m in ("greedy", "exact"):
                costs[m].append(float(pairing_cost(s, target, compute_ot_pairing(s, target, method=m))))
        alone = windows(pair, args.windows, args.reps, device)

        torch.manual_seed(0)
        tr = FlowTrainer(Unet(dim=args.dim, dim_mults=(1, 2, 4, 8), channels=4, n_classes=10).to(device), lr=1e-4)
        cond = {"class_cond": cls, "mask_cond": None}
        step = {m: (lambda r, m=m: tr.step(sources[r % len(sources)], target, cond,
                                           pairing=compute_ot_pairing(sources[r % len(sources)], target, method=m))) for m in ("greedy", "exact")}
        for m in step:
            for r in range(3):
                loss = step[m](r)
        steps = windows(step, args.windows, args.steps, device)
        assert bool(torch.isfinite(loss))
        a = {m: summary(alone[m]) for m in alone}
        s = {m: summary(steps[m]) for m in steps}
        allowed = s["greedy"]["median_ms"] + (a["exact"]["median_ms"] - a["greedy"]["median_ms"]) + s["greedy"]["spread_ms"]
        row = {"batch": B, "dim": 4096, "pairing_alone": a, "step": s,
               "pairing_cost": {k: round(statistics.mean(v), 3) for k, v in costs.items()},
               "exact_share_of_step": round(a["exact"]["median_ms"] / s["exact"]["median_ms"], 4),
               "criterion": {"step_exact_ms": s["exact"]["median_ms"], "allowed_ms": round(allowed, 4),
                             "met": bool(s["exact"]["median_ms"] <= allowed)}}
        results.append(row)
        print(json.dumps(row), flush=True)
        del tr
        torch.cuda.empty_cache()
    doc = {"tool": "tools/bench_ot.py", "device": torch.cuda.get_device_name(device),
           "inputs": "source N(0, I), target N(0, I) with a fixed seed, D = 4096 (4x32x32); solver work depends on the data",
           "model": f"U-Net dim={args.dim} dim_mults [1,2,4,8] n_classes=10, latents 4x32x32",
           "timing": f"{args.windows} alternating windows; {args.reps} pairing calls / {args.steps} steps per window; host clock around "
                     "device synchronisations; median, min, max, spread = max - min over windows",
           "criterion": "step(exact) <= step(greedy) + (exact alone - greedy alone) + spread of step(greedy)",
           "results": results, "criterion_met_everywhere": all(r["criterion"]["met"] for r in results)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}; criterion {'met' if doc['criterion_met_everywhere'] else 'MISSED'}")


if __name__ == "__main__":
    main()
