#!/usr/bin/env python3
"""Codebook fitting, measured: one training step of the residual quantiser (``fc_rvq_train_step``), ``fc_rvq_quantize`` alone (the same
search, the fixed part of the step), the same step written with torch operations on the device (``cdist`` / ``argmin``, ``bincount``,
``index_add_`` in fp64, the EMA lines; without dead-code expiry, which only the native step carries), the training call of the module
(``ResidualVQ.quantize_nchw`` in training mode: the step plus the stacking and copying of the per-level buffers), and one full
initialisation (per level: seed the codes, fifteen Lloyd iterations).  N = 16,384 and 65,536 latent vectors (B = 64 and 256 at 16 x 16) at
(D, K, L) = (4, 96, 4) and (4, 512, 4), Gaussian latents.

Every sample is the host time of ``reps`` back-to-back calls ending in a device synchronise, divided by ``reps``; the sides are sampled
alternately, ``samples`` times each; reported are the medians and the run-to-run spread (max - min over the samples) of each side.

The expectation is that the step is faster than the torch form at every shape: met when the step's slowest sample is below the torch
form's fastest.  Prints met or MISSED per shape and writes everything to ``profiles/rvq_fit_bench.json`` (``--out``)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DECAY, CW, THRESHOLD, ITERS, SEED = 0.95, 0.25, 2.0, 15, 0
SHAPES = [(64, 4, 96, 4), (256, 4, 96, 4), (64, 4, 512, 4), (256, 4, 512, 4)]       # (B, D, K, L) at 16 x 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rvq_fit_bench.json"))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--samples", type=int, default=9)
    args = ap.parse_args()

    import torch
    from flocoder_amd import _binding as B
    from flocoder_amd.codecs import ResidualVQ
    if not torch.cuda.is_available():
        raise SystemExit("bench_rvq_fit: no GPU; timings are taken on the MI355X only")
    dev = torch.device("cuda:0")
    lib = B.lib()

    def sample(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0) / reps

    def stats(v):
        return {"median_us": round(float(np.median(v)), 2), "min_us": round(float(min(v)), 2), "max_us": round(float(max(v)), 2),
                "spread_us": round(float(max(v) - min(v)), 2)}

    result = {"decay": DECAY, "threshold_ema_dead_code": THRESHOLD, "kmeans_iters": ITERS, "reps": args.reps, "samples": args.samples, "cases": []}
    for bsz, d, k, nl in SHAPES:
        hw, n = 256, bsz * 256
        torch.manual_seed(bsz + k)
        z = torch.randn(bsz, d, 16, 16, device=dev)
        stream = B.current_stream(dev)
        nbytes = lib.fc_rvq_train_workspace_bytes(bsz, hw, d, k, nl)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        cb, cs, ea = torch.zeros(nl, k, d, device=dev), torch.zeros(nl, k, device=dev), torch.zeros(nl, k, d, device=dev)
        zq, idx = torch.empty_like(z), torch.empty(n, nl, dtype=torch.int64, device=dev)
        losses, expired = torch.empty(nl, device=dev), torch.empty(nl, dtype=torch.int32, device=dev)
        shape = (bsz, d, hw, k, nl)

        def init():
            for lvl in range(nl):
                B.check(lib.fc_rvq_seed_codes(B.ptr(z), B.ptr(cb), *shape, lvl, SEED, 0, stream))
                B.check(lib.fc_rvq_kmeans(B.ptr(z), B.ptr(cb), *shape, lvl, ITERS, B.ptr(cs[lvl]), B.ptr(ea[lvl]), None, B.ptr(ws), nbytes, stream))

        def step():
            B.check(lib.fc_rvq_train_step(B.ptr(z), B.ptr(cb), B.ptr(cs), B.ptr(ea), B.ptr(zq), B.ptr(idx), B.ptr(losses), B.ptr(expired), *shape,
                                          DECAY, CW, THRESHOLD, SEED, 1, B.ptr(ws), nbytes, stream))

        def quantize():
            B.check(lib.fc_rvq_quantize(B.ptr(z), B.ptr(cb), B.ptr(zq), B.ptr(idx), *shape, stream))

        init()
        tcb, tcs, tea = cb.clone(), cs.clone(), ea.clone()
        flat = z.permute(0, 2, 3, 1).reshape(n, d).contiguous()

        def torch_step():
            r, new = flat, []
            for lvl in range(nl):
                e = tcb[lvl]
                i = torch.cdist(r, e).argmin(dim=1)
                q = e[i]
                cnt = torch.bincount(i, minlength=k)
                s = torch.zeros(k, d, dtype=torch.float64, device=dev).index_add_(0, i, r.double())
                commit = ((r - q).double() ** 2).sum()
                c64 = tcs[lvl].double().lerp_(cnt.double(), 1 - DECAY)
                a64 = tea[lvl].double().lerp_(s, 1 - DECAY)
                tcs[lvl].copy_(c64)
                tea[lvl].copy_(a64)
                c64, tot = tcs[lvl].double(), tcs[lvl].double().sum()
                new.append((tea[lvl].double() / ((c64 + 1e-5) / (tot + k * 1e-5) * tot)[:, None]).float())
                losses[lvl] = CW * commit / (n * d)
                r = r - q
            for lvl in range(nl):
                tcb[lvl].copy_(new[lvl])

        mod = ResidualVQ(d, k, nl, seed=SEED).to(dev).train()
        mod.quantize_nchw(z)                                                 # initialises; the timed calls are steps

        for fn in (step, quantize, torch_step, lambda: mod.quantize_nchw(z)):     # warm-up of every timed path at this shape
            sample(fn, 5)
        t = {"step": [], "quantize": [], "torch_step": [], "module_call": [], "init": []}
        for _ in range(args.samples):                                        # alternating, so a slow moment of the host meets every side
            t["step"].append(sample(step, args.reps))
            t["torch_step"].append(sample(torch_step, max(args.reps // 4, 1)))
            t["quantize"].append(sample(quantize, args.reps))
            t["module_call"].append(sample(lambda: mod.quantize_nchw(z), max(args.reps // 4, 1)))
            t["init"].append(sample(init, max(args.reps // 40, 1)))
        met = max(t["step"]) < min(t["torch_step"])
        case = {"batch": bsz, "vectors": n, "dim": d, "codebook_size": k, "levels": nl, **{key: stats(v) for key, v in t.items()},
                "torch_over_step": round(float(np.median(t["torch_step"]) / np.median(t["step"])), 2),
                "step_faster_than_torch": "met" if met else "MISSED"}
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
        print(f"N={n} K={k}: step {case['step']['median_us']} us (spread {case['step']['spread_us']}), torch form {case['torch_step']['median_us']} us "
              f"(spread {case['torch_step']['spread_us']}), quantize alone {case['quantize']['median_us']} us, module call "
              f"{case['module_call']['median_us']} us, initialisation {case['init']['median_us']} us: {'met' if met else 'MISSED'}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
