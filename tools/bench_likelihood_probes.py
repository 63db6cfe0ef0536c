#!/usr/bin/env python3
"""K Hutchinson probes in one likelihood solve against K single-probe calls, at the headline's model and batch: flowers-sized U-Net (dim
32, dim_mults [1,2,4,8], 102 classes), B = 64 latents of 4x32x32, class ids; the RK4 grid with --n-steps points and the adaptive solve
at rtol = atol = 1e-5 per sample.  The model's plans are in the training form throughout (no plan is rebuilt inside a timed call).
Writes ONE JSON line (profiles/likelihood_probes_bench.json) and prints every expectation as met or missed.

In one process, alternating within every repetition: for K in --ks the K-probe call T(K) and K single-probe calls in a row (the
probes are the K-probe call's); and, as tools/bench_likelihood.py times them, the chain alone (Unet.vjp_x over --inner calls) -- the
forward + chain evaluation is T(1) over its evaluations.

  expectation "k_probes"   T(K) <= T(1) nfe(K)/nfe(1) + (K - 1) nfe(K) t_chain + spread, per method and K: one forward per evaluation
                           and K chains behind it.  nfe is 4 (n_steps - 1) on the grid; adaptive: the call's largest nfev (the batch is
                           evaluated until its last sample finishes), which moves a little with the probes -- hence the ratio.
                           spread = max - min of T(1) over the repetitions.
  expectation "t1_parent"  T(1) of this build <= T(1) of the parent build + spread, from --ab: a file of the lines that --t1-only runs
                           of the two builds wrote, alternating, in the same session (the caller starts them: two trees, two libraries)
  logp_stderr              at K = 8, over the batch: median and maximum, in nats and in bits per dimension -- what a user needs to pick K

    python tools/bench_likelihood_probes.py [--reps 3] [--rk45-reps 2] [--ks 1,2,4,8] [--ab FILE]
    python tools/bench_likelihood_probes.py --t1-only --tag NAME        (one JSON line on stdout: T(1) of both methods, nothing written)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rk45-reps", type=int, default=2)
    ap.add_argument("--n-steps", type=int, default=50)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--ab", default=None)
    ap.add_argument("--t1-only", action="store_true")
    ap.add_argument("--tag", default="this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "likelihood_probes_bench.json"))
    a = ap.parse_args()
    from flocoder_amd import sampling as S
    from flocoder_amd.unet import Unet
    if not torch.cuda.is_available():
        sys.exit("bench_likelihood_probes needs an MI355X")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    ks = sorted({int(k) for k in a.ks.split(",")} | {1})
    shape = (BATCH,) + LATENT
    ids = torch.randint(NCLS, (BATCH,), generator=torch.Generator().manual_seed(1235)).to(dev)
    x0 = torch.randn(shape, generator=torch.Generator().manual_seed(1234)).to(dev)
    eps = (torch.randint(0, 2, (max(ks),) + shape, generator=torch.Generator().manual_seed(1236)).float() * 2 - 1).to(dev)
    model = Unet(dim=DIM, dim_mults=(1, 2, 4, 8), channels=LATENT[0], n_classes=NCLS).eval().to(dev)
    grid = S.rk4_time_grid(a.n_steps).flip(0)
    evals = 4 * (a.n_steps - 1)

    def rk4(probe):
        out = model.log_likelihood(x0.clone(), grid, probe, class_ids=ids, restore_plan=False)
        return out, evals

    def rk45(probe):
        out = model.log_likelihood_rk45(x0.clone(), probe, per_sample=True, class_ids=ids, restore_plan=False)
        return out[1:], int(out[0][0].max())

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out

    rk4(eps[0]); rk45(eps[0])                                # warm: plans, code objects
    if a.t1_only:
        t4 = [timed(lambda: rk4(eps[0]))[0] for _ in range(a.reps)]
        t5 = [timed(lambda: rk45(eps[0]))[0] for _ in range(a.reps)]
        print(json.dumps({"tag": a.tag, "rk4_t1_ms": [round(t * 1e3, 2) for t in t4], "rk45_t1_ms": [round(t * 1e3, 2) for t in t5]}), flush=True)
        return

    def sweep(call, reps):
        """per K: the K-probe call's times, the times of K single-probe calls in a row, the call's evaluations"""
        multi, singles, nfe, last = {k: [] for k in ks}, {k: [] for k in ks}, {}, {}
        for _ in range(reps):
            for k in ks:
                dt, (out, n) = timed(lambda: call(eps[0] if k == 1 else eps[:k]))
                multi[k].append(dt); nfe[k] = n; last[k] = out
                singles[k].append(timed(lambda: [call(eps[j]) for j in range(k)])[0])
        return multi, singles, nfe, last

    m4, s4, n4, o4 = sweep(rk4, a.reps)
    # the chain alone, as tools/bench_likelihood.py times it
    tvec = torch.full((BATCH,), 500.0, device=dev)
    model._forward_native(x0, tvec, ids, None, train=True)

    def only_dx():
        for _ in range(a.inner):
            model.vjp_x(x0, tvec, ids, eps[0])

    only_dx()
    t_chain = statistics.median(timed(only_dx)[0] / a.inner for _ in range(max(3, a.reps)))
    m5, s5, n5, o5 = sweep(rk45, a.rk45_reps)
    model.release_training_plan()

    ms = lambda v: statistics.median(v) * 1e3
    D = math.prod(LATENT)
    rec = {"tool": "bench_likelihood_probes", "device": torch.cuda.get_device_name(dev), "batch": BATCH, "latent": list(LATENT), "dim": DIM,
           "n_classes": NCLS, "n_steps": a.n_steps, "rtol": 1e-5, "atol": 1e-5, "reps": a.reps, "rk45_reps": a.rk45_reps,
           "AMD_DIRECT_DISPATCH": os.environ.get("AMD_DIRECT_DISPATCH"), "chain_ms": round(t_chain * 1e3, 4)}
    verdicts = []
    for name, multi, singles, nfe, last in (("rk4", m4, s4, n4, o4), ("rk45_per_sample", m5, s5, n5, o5)):
        t1, spread = ms(multi[1]), (max(multi[1]) - min(multi[1])) * 1e3
        part = {"t1_ms": round(t1, 2), "t1_spread_ms": round(spread, 2), "eval_ms": round(t1 / nfe[1], 4), "by_k": {}}
        for k in ks:
            limit = t1 * nfe[k] / nfe[1] + (k - 1) * nfe[k] * t_chain * 1e3 + spread
            e = {"evaluations": nfe[k], "t_ms": round(ms(multi[k]), 2), "t_spread_ms": [round(min(multi[k]) * 1e3, 2), round(max(multi[k]) * 1e3, 2)],
                 "k_single_calls_ms": round(ms(singles[k]), 2), "ratio_vs_k_calls": round(ms(multi[k]) / ms(singles[k]), 4),
                 "limit_ms": round(limit, 2), "expectation": "met" if ms(multi[k]) <= limit else "missed"}
            part["by_k"][str(k)] = e
            verdicts.append(f"{name} K={k}: T(K) {e['t_ms']} ms, limit {e['limit_ms']} ms, {e['ratio_vs_k_calls']} of {k} calls: {e['expectation']}")
        se = last[ks[-1]][-1]
        part["logp_stderr_at_k"] = ks[-1]
        part["logp_stderr_nats"] = {"median": float(se.median()), "max": float(se.max())}
        part["logp_stderr_bits_per_dim"] = {"median": float(se.median()) / (D * math.log(2.0)), "max": float(se.max()) / (D * math.log(2.0))}
        rec[name] = part
    if a.ab:
        runs = [json.loads(line) for line in open(a.ab) if line.strip().startswith("{")]
        ab = {}
        for key, name in (("rk4_t1_ms", "rk4"), ("rk45_t1_ms", "rk45_per_sample")):
            new = [t for r in runs if r["tag"] == "this" for t in r[key]]
            old = [t for r in runs if r["tag"] == "parent" for t in r[key]]
            spread = max(new) - min(new)
            ok = statistics.median(new) <= statistics.median(old) + spread
            ab[name] = {"this_ms": new, "parent_ms": old, "this_median_ms": statistics.median(new), "parent_median_ms": statistics.median(old),
                        "spread_ms": round(spread, 2), "expectation": "met" if ok else "missed"}
            verdicts.append(f"{name} T(1): this build {statistics.median(new)} ms, parent {statistics.median(old)} ms, spread {spread:.2f} ms: {ab[name]['expectation']}")
        rec["t1_vs_parent"] = ab
    line = json.dumps(rec)
    print(line, flush=True)
    print("\n".join(verdicts), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
