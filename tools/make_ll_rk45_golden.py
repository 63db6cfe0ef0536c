#!/usr/bin/env python3
"""tests/golden/ll_rk45_scipy_oracle.npz: the adaptive (RK45) flow log-likelihood, the contract of fc_unet_log_likelihood_rk45
(tests/test_gpu_likelihood_rk45.py).  tests/likelihood_rk45_ref.py -- scipy's RK45 on the concatenated state [x, a] around the fp64
oracle U-Net under autograd -- solves every case of its CASES from t = 1 to t = 0 at rtol = atol = 1e-5 in both modes: "coupled" (one
controller group over the batch) and "ps" (one group per sample).  Inputs are named by case and seed (likelihood_rk45_ref.case_inputs, which also says how the cases were chosen);
stored per case and mode: z, a, logp, counts ([G, 3]: nfev, accepted, rejected), gsum and margin ([G]), and per case ``a_tight``: a of a per-sample
solve at rtol = atol = TIGHT, the yardstick of the solves' own integration error; per case and mode ``z32_rel`` / ``counts32``: the same
solve over the fp32 oracle against the fp64 one (relative L2 of z per sample, its counters), by which the cases were admitted.

    python tools/make_ll_rk45_golden.py        (minutes on the host: one process per solve)
"""
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import likelihood_rk45_ref as rr  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ll_rk45_scipy_oracle.npz")
TIGHT = 1e-7


def solve(job):
    cid, mode, tol = job
    torch.set_num_threads(1)
    sd, x, eps, cond = rr.case_inputs(cid)
    if tol == "fp32":        # the same solve with every evaluation in fp32: how far the case's z moves with the evaluation's precision
        r = rr.log_likelihood_rk45_ref(sd, x, cond, eps, per_sample=mode == "ps", rtol=rr.RTOL, atol=rr.ATOL)
    else:
        sd64 = {k: v.double() for k, v in sd.items()}
        r = rr.log_likelihood_rk45_ref(sd64, x.double(), cond, eps.double(), per_sample=mode == "ps", rtol=tol, atol=tol)
    return job, {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in r._asdict().items()}


def main():
    jobs = [(cid, mode, tol) for cid in rr.CASES for mode in ("coupled", "ps") for tol in (rr.RTOL, "fp32")] + [(cid, "ps", TIGHT) for cid in rr.CASES]
    z32 = {}
    out = {"tight_tol": np.float64(TIGHT), "tol": np.float64(rr.RTOL)}
    with ProcessPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1)) as pool:
        for (cid, mode, tol), r in pool.map(solve, jobs):
            if tol == "fp32":
                z32[(cid, mode)] = r
            elif tol == TIGHT:
                out[f"{cid}.a_tight"] = r["a"]
                out[f"{cid}.counts_tight"] = r["counts"]
            else:
                for k, v in r.items():
                    out[f"{cid}.{mode}.{k}"] = v
            print(json.dumps({"case": cid, "mode": mode, "tol": tol, "counts": r["counts"].tolist(), "a": r["a"].tolist()}), flush=True)
    for (cid, mode), r in z32.items():
        z, zr = r["z"].astype(np.float64).reshape(len(r["z"]), -1), out[f"{cid}.{mode}.z"].reshape(len(r["z"]), -1)
        out[f"{cid}.{mode}.z32_rel"] = np.linalg.norm(z - zr, axis=1) / np.linalg.norm(zr, axis=1)
        out[f"{cid}.{mode}.counts32"] = r["counts"]
        print(json.dumps({"case": cid, "mode": mode, "z32_rel": out[f"{cid}.{mode}.z32_rel"].tolist(), "counts32": r["counts"].tolist()}), flush=True)
    np.savez_compressed(OUT, **out)


if __name__ == "__main__":
    main()
