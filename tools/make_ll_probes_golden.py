#!/usr/bin/env python3
"""tests/golden/ll_probes_rk45_scipy_oracle.npz: the K-probe adaptive (RK45) flow log-likelihood, the contract of
fc_unet_log_likelihood_rk45_probes (tests/test_gpu_likelihood_probes.py).  tests/likelihood_probes_ref.py -- tests/likelihood_rk45_ref.py's
stepping of scipy's RK45 on [x, a] around the fp64 oracle U-Net, with da/dt the mean of K = 3 probes' estimates -- solves the two cases of
the single-probe golden (same models, latents, tolerances and first probe; two more probes from fixed seeds) in both modes.  Stored
per case and mode: what tools/make_ll_rk45_golden.py stores (z, a, logp, counts, gsum [K, B], margin, z32_rel, counts32) plus
``a_probes`` [K, B]; per case ``a_tight`` (a of a per-sample solve with the same probes at rtol = atol = TIGHT) and ``probe_seeds``.

Admission is the single-probe golden's (likelihood_rk45_ref.FP32_AGREEMENT): every solve of a case -- both modes, every sample -- must
agree between the fp32 and the fp64 oracle to FP32_AGREEMENT in z with equal counters and must contain rejected steps; a case that
fails is tried with the next pair of probe seeds of CANDIDATES, and nothing is written unless every case is admitted.  Tried so far
(the admitted pair is likelihood_probes_ref.PROBE_SEEDS):
    d16c10-class  (101, 102) not admitted (z32_rel up to 1.5e-4 per sample, 1.1e-4 coupled; counters equal); (103, 104) admitted
    d8mask        (101, 102) and (103, 104) not admitted (per sample: counters 560 / 536 against 506 evaluations in one sample, z32_rel up to
                  1e-2; coupled admitted both times); (105, 106) admitted

    python tools/make_ll_probes_golden.py        (minutes on the host: one process per solve)
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

import likelihood_probes_ref as pr  # noqa: E402
import likelihood_rk45_ref as rr  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ll_probes_rk45_scipy_oracle.npz")
TIGHT = 1e-7
# probe seed pairs per case, in the order tried
CANDIDATES = {cid: [(101, 102), (103, 104), (105, 106), (107, 108)] for cid in rr.CASES}


def solve(job):
    cid, seeds, mode, tol = job
    torch.set_num_threads(1)
    sd, x, eps, cond = pr.case_inputs(cid, seeds)
    if tol == "fp32":
        r = pr.log_likelihood_probes_ref(sd, x, cond, eps, per_sample=mode == "ps", rtol=rr.RTOL, atol=rr.ATOL)
    else:
        sd64 = {k: v.double() for k, v in sd.items()}
        r = pr.log_likelihood_probes_ref(sd64, x.double(), cond, eps.double(), per_sample=mode == "ps", rtol=tol, atol=tol)
    return job, {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in r._asdict().items()}


def admit(pool, cid, seeds):
    """The case's record with these probe seeds, or None if a solve fails admission."""
    jobs = [(cid, seeds, mode, tol) for mode in ("coupled", "ps") for tol in (rr.RTOL, "fp32")]
    res = dict(pool.map(solve, jobs))
    rec, ok = {}, True
    for mode in ("coupled", "ps"):
        r, r32 = res[(cid, seeds, mode, rr.RTOL)], res[(cid, seeds, mode, "fp32")]
        z, zr = r32["z"].astype(np.float64).reshape(len(r["z"]), -1), r["z"].reshape(len(r["z"]), -1)
        rel = np.linalg.norm(z - zr, axis=1) / np.linalg.norm(zr, axis=1)
        good = bool((rel <= rr.FP32_AGREEMENT).all() and np.array_equal(r32["counts"], r["counts"]) and (r["counts"][:, 2] >= 1).all())
        print(json.dumps({"case": cid, "seeds": seeds, "mode": mode, "counts": r["counts"].tolist(), "counts32": r32["counts"].tolist(),
                          "z32_rel": rel.tolist(), "a": r["a"].tolist(), "a_probes": r["a_probes"].tolist(), "admitted": good}), flush=True)
        ok = ok and good
        for k, v in r.items():
            rec[f"{cid}.{mode}.{k}"] = v
        rec[f"{cid}.{mode}.z32_rel"], rec[f"{cid}.{mode}.counts32"] = rel, r32["counts"]
    return rec if ok else None


def main():
    out = {"tight_tol": np.float64(TIGHT), "tol": np.float64(rr.RTOL)}
    with ProcessPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        for cid in rr.CASES:
            for seeds in CANDIDATES[cid][CANDIDATES[cid].index(tuple(pr.PROBE_SEEDS[cid])):]:   # (earlier pairs: tried, see above)
                rec = admit(pool, cid, seeds)
                if rec is not None:
                    break
            else:
                sys.exit(f"{cid}: no candidate probe seeds admitted; nothing written")
            if tuple(seeds) != tuple(pr.PROBE_SEEDS[cid]):
                sys.exit(f"{cid}: admitted with seeds {seeds}; set likelihood_probes_ref.PROBE_SEEDS and run again")
            out.update(rec)
            out[f"{cid}.probe_seeds"] = np.array(seeds, dtype=np.int64)
            _, r = solve((cid, seeds, "ps", TIGHT))
            out[f"{cid}.a_tight"], out[f"{cid}.counts_tight"], out[f"{cid}.a_probes_tight"] = r["a"], r["counts"], r["a_probes"]
            print(json.dumps({"case": cid, "tight": r["a"].tolist(), "counts": r["counts"].tolist()}), flush=True)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
