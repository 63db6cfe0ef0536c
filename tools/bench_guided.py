#!/usr/bin/env python3
"""Measurement-guided sampling at the headline's model and batch: flowers-sized U-Net (dim 32, dim_mults [1,2,4,8], 102 classes, weights
seeded as bench.py seeds them), B=64 latents of 4x32x32, class ids, n_steps=50, init_strength=0.2 (40 grid points, 156 evaluations).
Calls alternate in one process.  Prints ONE JSON line (profiles/guided_bench.json):

  identity_ms_per_eval     sampling.generate_latents_guided(jacobian="identity", cfg_strength=3): the captured RK4 step with guided stage
                           kernels (median of --reps calls over the call's true 4 (points - 1) evaluations)
  rk4_ms_per_eval          sampling.generate_latents_rk4 with the same init_latents / init_strength / cfg_strength on the same model: the
                           path the guided one extends; identity_over_rk4 = their ratio
  exact_ms_per_eval        Unet.integrate_guided(jacobian="exact") without guidance on a model whose plans are in the training form already
                           (restore_plan=False: no plan is rebuilt inside the timed call): per evaluation a training-form forward, the w
                           kernel, the backward plan's data-gradient chain and one stage kernel
  ll_ms_per_eval           sampling.log_likelihood on that model (50 grid points): the same forward + chain per evaluation;
                           exact_over_ll = their ratio
The tool fails only if the identity form is slower than the plain sampler by more than the spread (max - min) of the plain sampler's own
timings in this run.  (Measured on the MI355X, profiles/guided_bench.json: identity 324.08 ms against 322.43 ms, 1.005x, with a plain-sampler
spread of 0.60 ms -- the criterion is missed by about 1 ms per call, ~10 us per guided stage kernel; exact 0.98x the likelihood.)

    python tools/bench_guided.py [--reps 5] [--n-steps 50]
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
INIT_STRENGTH, CFG = 0.2, 3.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-steps", type=int, default=50)
    a = ap.parse_args()
    from flocoder_amd import sampling as S
    from flocoder_amd.unet import Unet
    if not torch.cuda.is_available():
        sys.exit("bench_guided needs an MI355X")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    shape = (BATCH,) + LATENT
    gen = lambda seed: torch.Generator().manual_seed(seed)
    ids = torch.randint(NCLS, (BATCH,), generator=gen(1235)).to(dev)
    src = torch.randn(shape, generator=gen(1234)).to(dev)
    known = torch.randn(shape, generator=gen(1237)).to(dev)
    keep = (torch.rand((BATCH, 1) + LATENT[1:], generator=gen(1238)) > 0.4).float().to(dev)
    y = keep * known
    eps = (torch.randint(0, 2, shape, generator=gen(1236)).float() * 2 - 1).to(dev)
    cond = {"class_cond": ids}
    # two models with the same weights: `sampler_model` keeps inference-form plans (identity form and the plain sampler), `model` is put
    # into the training form once (exact form and the likelihood), so that no timed call rebuilds a plan
    sampler_model = Unet(dim=DIM, dim_mults=(1, 2, 4, 8), channels=LATENT[0], n_classes=NCLS).eval().to(dev)
    model = sampler_model.replica()
    model._forward_native(src, torch.full((BATCH,), 500.0, device=dev), ids, None, train=True)
    ts = S.rk4_time_grid(a.n_steps, INIT_STRENGTH)
    evals = 4 * (len(ts) - 1)
    ll_evals = 4 * (a.n_steps - 1)

    def identity():
        return S.generate_latents_guided(sampler_model, shape, y, keep, n_steps=a.n_steps, init_strength=INIT_STRENGTH, cond=cond,
                                         cfg_strength=CFG, source=src)[0]

    def rk4():
        return S.generate_latents_rk4(sampler_model, shape, a.n_steps, cond, CFG, source=src, init_latents=y, init_strength=INIT_STRENGTH)[0]

    def exact():
        x = ((1 - INIT_STRENGTH) * src + INIT_STRENGTH * y).contiguous()
        return model.integrate_guided(x, ts, y, keep, jacobian="exact", class_ids=ids, restore_plan=False)

    def ll():
        return S.log_likelihood(model, src, n_steps=a.n_steps, cond=cond, probe=eps)[0]

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out

    outs = [fn() for fn in (identity, rk4, exact, ll)]             # warm: plans, graphs, code objects
    assert all(bool(torch.isfinite(o).all()) for o in outs)
    res = lambda lat: float((keep * (lat - known)).flatten(1).norm(dim=1).mean())
    t_id, t_rk, t_ex, t_ll = [], [], [], []
    for _ in range(a.reps):
        t_id.append(timed(identity)[0])
        t_rk.append(timed(rk4)[0])
        t_ex.append(timed(exact)[0])
        t_ll.append(timed(ll)[0])
    ms = lambda v: statistics.median(v) * 1e3
    spread = lambda v: [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)]
    rec = {"tool": "bench_guided", "device": torch.cuda.get_device_name(dev), "batch": BATCH, "latent": list(LATENT), "dim": DIM,
           "n_classes": NCLS, "n_steps": a.n_steps, "init_strength": INIT_STRENGTH, "grid_points": len(ts), "evaluations": evals,
           "cfg_strength_identity": CFG, "reps": a.reps, "AMD_DIRECT_DISPATCH": os.environ.get("AMD_DIRECT_DISPATCH"),
           "identity_ms_per_call": round(ms(t_id), 2), "identity_ms_per_eval": round(ms(t_id) / evals, 4),
           "rk4_ms_per_call": round(ms(t_rk), 2), "rk4_ms_per_eval": round(ms(t_rk) / evals, 4),
           "identity_over_rk4": round(ms(t_id) / ms(t_rk), 4),
           "identity_spread_ms": spread(t_id), "rk4_spread_ms": spread(t_rk),
           "exact_ms_per_call": round(ms(t_ex), 2), "exact_ms_per_eval": round(ms(t_ex) / evals, 4),
           "ll_ms_per_call": round(ms(t_ll), 2), "ll_evaluations": ll_evals, "ll_ms_per_eval": round(ms(t_ll) / ll_evals, 4),
           "exact_over_ll": round((ms(t_ex) / evals) / (ms(t_ll) / ll_evals), 4),
           "exact_spread_ms": spread(t_ex), "ll_spread_ms": spread(t_ll),
           "kept_residual_mean": {"identity": round(res(outs[0]), 3), "unguided": round(res(outs[1]), 3), "exact": round(res(outs[2]), 3)}}
    print(json.dumps(rec), flush=True)
    slack = (max(t_rk) - min(t_rk)) * 1e3
    if ms(t_id) > ms(t_rk) + slack:
        sys.exit(f"identity form {ms(t_id):.2f} ms per call against the plain sampler's {ms(t_rk):.2f} ms: slower by more than the plain "
                 f"sampler's own spread ({slack:.2f} ms)")


if __name__ == "__main__":
    main()
