#!/usr/bin/env python3
"""What the entropic (Sinkhorn) OT plan costs and buys: D = 4096 (the stl_sd.yaml latent, 4x32x32), B = 64, 128, 256, reg = 0.05 and
0.01 on the normalised cost, the Gaussian source / fixed-seed Gaussian target batches of tools/bench_ot.py (the iteration count depends
on the data: these figures are for that input).

    python tools/bench_ot_plan.py [--batches 64 128 256 --regs 0.05 0.01 --reps 20 --steps 20 --windows 5 --out profiles/ot_plan_bench.json]

Per batch size and reg: the iterations to convergence (over the sources), the time per compute_ot_plan call, per call of the solver
alone on the finished matrix and per iteration of that, and the same iteration written with torch.logsumexp on the device in fp64 --
what a user would otherwise write -- run for the same number of iterations without any stopping check.  The per-iteration figures
divide a window's median time per call by the mean iteration count of the sources, while the calls cycle through the sources with
their own counts: exact when all counts are equal (iterations_min = iterations_max), an average otherwise.
Per batch size: pairing_cost of the identity, greedy, sinkhorn (per reg) and exact pairings, and
FlowTrainer.step (U-Net dim 32, the coupling computed inside the step) with the greedy pairing, the sinkhorn pairing and pairs sampled
from the plan (reg 0.05), timed as bench_ot.py times them.  Expectations, reported as met or MISSED:
  - time per iteration below the torch loop's at every B and reg (the loop is several launches per half iteration, the kernel none);
  - step(x) <= step(greedy) + (x alone - greedy alone) + the spread of step(greedy), x = sinkhorn, sinkhorn_sample: the new paths add
    their own kernels' time and no hidden synchronisation or stall."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_ot import summary, windows  # noqa: E402


def torch_loop(cost, reg, iterations):
    """The solver's iteration with torch.logsumexp, fp64 as the kernel, no stopping check."""
    c = cost.double()
    n = c.shape[0]
    lb = -math.log(n)
    f = torch.full((n,), reg * lb, device=c.device, dtype=torch.float64)
    g = f.clone()
    for _ in range(iterations):
        g = reg * (lb - torch.logsumexp((f[:, None] - c) / reg, 0))
        f = reg * (lb - torch.logsumexp((g[None, :] - c) / reg, 1))
    return torch.exp((f[:, None] + g[None, :] - c) / reg).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--regs", type=float, nargs="+", default=[0.05, 0.01])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--sources", type=int, default=8)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ot_plan_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ot_plan.py measures on an MI355X; no GPU found")
    from flocoder_amd._ops import ot_sinkhorn
    from flocoder_amd.ot import compute_ot_pairing, compute_ot_plan, pairing_cost, sample_plan
    from flocoder_amd.train import FlowTrainer
    from flocoder_amd.unet import Unet
    device = torch.device("cuda", 0)
    results = []
    for B in args.batches:
        g = torch.Generator().manual_seed(1234 + B)
        target = torch.randn(B, 4, 32, 32, generator=g).to(device)
        sources = [torch.randn(B, 4, 32, 32, generator=g).to(device) for _ in range(args.sources)]
        cls = torch.randint(10, (B,), generator=g).to(device)
        src = lambda r: sources[r % len(sources)]
        costs = {"identity": [], "greedy": [], "exact": []}
        for s in sources:
            costs["identity"].append(float(pairing_cost(s, target)))
            for m in ("greedy", "exact"):
                costs[m].append(float(pairing_cost(s, target, compute_ot_pairing(s, target, method=m))))
        plans = []
        for reg in args.regs:
            its, conv, errs, mats = [], [], [], []
            costs[f"sinkhorn_reg{reg}"] = []
            for s in sources:                                  # also the warm-up at this shape
                _, info = compute_ot_plan(s, target, reg=reg, normalize_cost=True, return_info=True)
                its.append(int(info["iterations"]))
                conv.append(bool(info["converged"]))
                errs.append(float(info["err"]))
                mats.append(info["cost"])
                perm = compute_ot_pairing(s, target, method="sinkhorn", reg=reg, normalize_cost=True)
                costs[f"sinkhorn_reg{reg}"].append(float(pairing_cost(s, target, perm)))
            n_it = int(round(statistics.mean(its)))
            torch_loop(mats[0], reg, 2)
            t = windows({"plan": lambda r: compute_ot_plan(src(r), target, reg=reg, normalize_cost=True),
                         "solver": lambda r: ot_sinkhorn(mats[r % len(mats)], reg),
                         "torch_loop": lambda r: torch_loop(mats[r % len(mats)], reg, its[r % len(its)])}, args.windows, args.reps, device)
            k, sv, tl = summary(t["plan"]), summary(t["solver"]), summary(t["torch_loop"])
            plans.append({"reg": reg, "iterations_mean": round(statistics.mean(its), 1), "iterations_min": min(its), "iterations_max": max(its),
                          "converged_all": all(conv), "err_max": max(errs), "plan_call": k, "solver_call": sv, "torch_loop_call": tl,
                          "us_per_iteration": round(1e3 * sv["median_ms"] / n_it, 3),
                          "torch_us_per_iteration": round(1e3 * tl["median_ms"] / n_it, 3),
                          "faster_than_torch_loop": bool(sv["median_ms"] < tl["median_ms"]),
                          "note": "plan_call = distance matrix, normalisation and solver; solver_call and torch_loop_call start from the matrix; "
                                  "the solver's time includes its checks (every 10th iteration) and writing the plan, the loop's has no check"})

        couple = {
            "greedy": lambda r: (src(r), cls, compute_ot_pairing(src(r), target, method="greedy")),
            "sinkhorn": lambda r: (src(r), cls, compute_ot_pairing(src(r), target, method="sinkhorn", reg=0.05, normalize_cost=True)),
        }

        def sampled(r):
            i, j = sample_plan(compute_ot_plan(src(r), target, reg=0.05, normalize_cost=True), seed=0, draw_index=r)
            return src(r)[i], cls[j], j
        couple["sinkhorn_sample"] = sampled
        alone = windows(couple, args.windows, args.reps, device)

        torch.manual_seed(0)
        tr = FlowTrainer(Unet(dim=args.dim, dim_mults=(1, 2, 4, 8), channels=4, n_classes=10).to(device), lr=1e-4)

        def make_step(fn):
            def run(r):
                s, c, pairing = fn(r)
                return tr.step(s, target, {"class_cond": c, "mask_cond": None}, pairing=pairing)
            return run
        step = {m: make_step(fn) for m, fn in couple.items()}
        for m in step:
            for r in range(3):
                loss = step[m](r)
        steps = windows(step, args.windows, args.steps, device)
        assert bool(torch.isfinite(loss))
        a = {m: summary(alone[m]) for m in alone}
        s = {m: summary(steps[m]) for m in steps}
        crit = {}
        for m in ("sinkhorn", "sinkhorn_sample"):
            allowed = s["greedy"]["median_ms"] + (a[m]["median_ms"] - a["greedy"]["median_ms"]) + s["greedy"]["spread_ms"]
            crit[m] = {"step_ms": s[m]["median_ms"], "allowed_ms": round(allowed, 4), "met": bool(s[m]["median_ms"] <= allowed)}
        row = {"batch": B, "dim": 4096, "plans": plans, "coupling_alone": a, "step": s,
               "pairing_cost": {k: round(statistics.mean(v), 3) for k, v in costs.items()}, "criterion": crit}
        results.append(row)
        print(json.dumps(row), flush=True)
        del tr
        torch.cuda.empty_cache()
    faster = all(p["faster_than_torch_loop"] for r in results for p in r["plans"])
    no_stall = all(c["met"] for r in results for c in r["criterion"].values())
    doc = {"tool": "tools/bench_ot_plan.py", "device": torch.cuda.get_device_name(device),
           "inputs": "source N(0, I), target N(0, I) with a fixed seed, D = 4096 (4x32x32), cost normalised by its maximum; the iteration "
                     "count depends on the data",
           "model": f"U-Net dim={args.dim} dim_mults [1,2,4,8] n_classes=10, latents 4x32x32",
           "timing": f"{args.windows} alternating windows; {args.reps} calls / {args.steps} steps per window; host clock around device "
                     "synchronisations; median, min, max, spread = max - min over windows",
           "expectations": {"per iteration faster than the torch.logsumexp loop at every batch and reg": "met" if faster else "MISSED",
                            "step(x) <= step(greedy) + (x alone - greedy alone) + spread of step(greedy)": "met" if no_stall else "MISSED"},
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}; torch-loop expectation {'met' if faster else 'MISSED'}; step expectation {'met' if no_stall else 'MISSED'}")


if __name__ == "__main__":
    main()
