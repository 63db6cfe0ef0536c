#!/usr/bin/env python3
"""Stochastic (SDE) sampling at the headline's model and batch: flowers-sized U-Net (dim 32, dim_mults [1,2,4,8], 102 classes, weights
seeded as bench.py seeds them), B=64 latents of 4x32x32, 65 grid points (64 intervals), sigma = 1, generated noise.  Calls alternate in
one process.  Prints ONE JSON line and writes it to --out (default profiles/sde_bench.json), every figure the median of --reps calls in ms per U-Net evaluation (a
guided pair counts once):

  em_ms_per_eval / em_cfg_ms_per_eval      sampling.generate_latents_sde(method="euler_maruyama") without / with cfg_strength=3
  heun_ms_per_eval                         method="heun" without guidance (128 evaluations)
  euler_ms_per_eval / euler_cfg_...        sampling.euler_sampler(sample_N=64) on the same model: the deterministic path with the same
                                           launch structure (with guidance) and the headline's fused step (without)
  parent_euler_...                         the same two figures measured on the parent commit (--parent-euler-ms / --parent-euler-cfg-ms;
                                           recorded, not gated)
  torch_em_ms_per_eval                     the same Euler-Maruyama call through the torch path: the model wrapped in a plain nn.Module, so
                                           one Python-level U-Net call per evaluation and the noise from fc_ode_normal_field -- what
                                           stochastic sampling cost before; torch_over_native = their ratio
Criterion: with guidance the SDE step has the Euler step's launch structure (time kernel, plan, update kernel), so em_cfg_ms_per_eval must
not exceed euler_cfg_ms_per_eval by more than the spread (max - min) of the Euler+CFG timings of this run.  Without guidance the step
carries two small launches the fused Euler tail does not; their cost (em - euler) is reported, not gated.  The tool states a miss and
exits non-zero.  (Measured on the MI355X, profiles/sde_bench.json: 2.087 against 2.071 ms with a spread of 0.0065 -- the criterion is
missed by 16 us per interval, the cost of generating the normals in the update kernel; without guidance 1.232 against 1.214; the torch
path 1.786, 1.45x.)

    python tools/bench_sde.py [--reps 5] [--parent-euler-ms X --parent-euler-cfg-ms Y] [--out profiles/sde_bench.json]
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
POINTS, CFG, SIGMA = 65, 3.0, 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-euler-ms", type=float, default=None)
    ap.add_argument("--parent-euler-cfg-ms", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sde_bench.json"))
    ap.add_argument("--euler-only", action="store_true", help="time the two Euler figures alone (what a parent checkout can run)")
    a = ap.parse_args()
    if a.reps < 5:
        sys.exit("bench_sde: the criterion is read against the spread of at least 5 repeats")
    from flocoder_amd import sampling as S
    from flocoder_amd.unet import Unet
    if not torch.cuda.is_available():
        sys.exit("bench_sde needs an MI355X")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    shape = (BATCH,) + LATENT
    gen = lambda seed: torch.Generator().manual_seed(seed)
    ids = torch.randint(NCLS, (BATCH,), generator=gen(1235)).to(dev)
    src = torch.randn(shape, generator=gen(1234)).to(dev)
    cond = {"class_cond": ids}
    # one handle per workload, all with the same weights: a plan is built for its reserved rows (64 without guidance: the headline's plan;
    # 128 with it), and a handle's captured graphs bake the position of its conditioning table, which moves with the number of evaluations
    # of a call -- workloads that alternate on one handle would re-capture their graphs on every call
    model = Unet(dim=DIM, dim_mults=(1, 2, 4, 8), channels=LATENT[0], n_classes=NCLS).eval().to(dev)

    class Wrapped(torch.nn.Module):                          # not a flocoder_amd.Unet: the samplers take their torch path
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, x, t, cond=None):
            return self.inner(x, t, cond)

    n_int = POINTS - 1
    sde = lambda m, method, cfg: S.generate_latents_sde(m, shape, n_steps=POINTS, cond=cond, cfg_strength=cfg, source=src, sigma=SIGMA,
                                                        method=method, seed=7)[0]
    euler = lambda m, cfg: S.euler_sampler(m, shape, n_int, cond=cond, source=src, cfg_strength=cfg)[0]

    def workload(fn, evals):
        m = model.replica()
        return (lambda: fn(m)), evals

    runs = {"euler": workload(lambda m: euler(m, 0.0), n_int), "euler_cfg": workload(lambda m: euler(m, CFG), n_int)}
    if not a.euler_only:
        runs.update({"em": workload(lambda m: sde(m, "euler_maruyama", 0.0), n_int),
                     "em_cfg": workload(lambda m: sde(m, "euler_maruyama", CFG), n_int),
                     "heun": workload(lambda m: sde(m, "heun", 0.0), 2 * n_int),
                     "torch_em": workload(lambda m: sde(Wrapped(m), "euler_maruyama", 0.0), n_int)})

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out

    outs = {k: fn() for k, (fn, _) in runs.items()}           # warm: plans, graphs, code objects
    assert all(bool(torch.isfinite(o).all()) for o in outs.values())
    times = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, (fn, _) in runs.items():
            times[k].append(timed(fn)[0])
    per_eval = lambda k: statistics.median(times[k]) * 1e3 / runs[k][1]
    spread = lambda k: (max(times[k]) - min(times[k])) * 1e3 / runs[k][1]
    rec = {"tool": "bench_sde", "device": torch.cuda.get_device_name(dev), "batch": BATCH, "latent": list(LATENT), "dim": DIM,
           "n_classes": NCLS, "grid_points": POINTS, "sigma": SIGMA, "cfg_strength": CFG, "reps": a.reps,
           "AMD_DIRECT_DISPATCH": os.environ.get("AMD_DIRECT_DISPATCH"),
           "parent_euler_ms_per_eval": a.parent_euler_ms, "parent_euler_cfg_ms_per_eval": a.parent_euler_cfg_ms}
    for k in runs:
        rec[f"{k}_ms_per_eval"] = round(per_eval(k), 4)
        rec[f"{k}_spread_ms_per_eval"] = round(spread(k), 4)
    miss = None
    if not a.euler_only:
        rec["em_minus_euler_ms_per_eval"] = round(per_eval("em") - per_eval("euler"), 4)
        rec["em_cfg_minus_euler_cfg_ms_per_eval"] = round(per_eval("em_cfg") - per_eval("euler_cfg"), 4)
        rec["torch_over_native"] = round(per_eval("torch_em") / per_eval("em"), 3)
        rec["criterion_met"] = per_eval("em_cfg") <= per_eval("euler_cfg") + spread("euler_cfg")
        if not rec["criterion_met"]:
            miss = (f"MISS: Euler-Maruyama with guidance {per_eval('em_cfg'):.4f} ms per evaluation against Euler with guidance "
                    f"{per_eval('euler_cfg'):.4f}: slower by more than that path's own spread ({spread('euler_cfg'):.4f})")
    print(json.dumps(rec), flush=True)
    if not a.euler_only:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(rec) + "\n")
    if miss:
        sys.exit(miss)


if __name__ == "__main__":
    main()
