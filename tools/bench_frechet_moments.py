#!/usr/bin/env python3
"""The moment form of the Frechet distance on the device, measured (flocoder_amd.distances.FrechetMoments; csrc/frechet.hip).

    python tools/bench_frechet_moments.py [--windows 3 --old-windows 2 --out profiles/frechet_moments_bench.json]

Two sets of N feature rows each in D dimensions (Gaussian rows through a fixed dense mixing (I + G / (2 sqrt(D))) diag(1 / sqrt(1 + j)):
a full-rank, dense covariance whose eigenvalues fall by about four decades at D = 2048; the condition number is reported, because the
factor's sweeps grow with it -- DESIGN.md section 4), resident on the device and fed in batches: (N, D, batch) = (50 000, 2048, 1000)
and (8192, 512, 256).

* ``FrechetMoments.update`` per batch (a whole pass over one set, divided by its batches) and its rate at the batch x D x (D + 1)
  operations of the lower triangle it computes -- the whole update (batch mean, mean join, scatter), not the scatter kernel alone;
  next to it torch's fp64 ``f.t() @ f`` of the same batch (conversion to fp64 included, as ``FrechetStatistics.update`` pays it) at
  2 x batch x D x D operations;
* ``factor()`` of one state (cache dropped before every call), with its sweeps and launches;
* ``frechet_distance_moments`` with no factor cached (three solves), with the real side's cached (two) and with both cached (one);
* the existing path on the same batches: ``metrics.FrechetStatistics.update`` over both sets, then ``metrics.frechet_distance`` (the
  product of the covariances to the host, ``torch.linalg.eigvals`` there); both values and their difference;
* ``fid_score(solver="moments")`` on 20 000 images per side with a 64-feature extractor, a set the sample form refuses.

Every sample is the host time of calls ending in a device synchronise (the distance calls end in the host's read of the result); the
sides alternate window by window; medians and the spread (max - min over the windows) are reported.

Expectations, each reported as met or MISSED:
(a) at D = 2048 the whole evaluation (both sets' updates and the distance, nothing cached) is faster than the existing path (both
    sets' updates and frechet_distance): slowest window of the new against the fastest of the old;
(b) with the real side's factor cached the distance costs two solves, not three: its launches are the uncached call's minus the
    real factor's, and its slowest window is faster than the uncached call's fastest;
(c) recorded only: the update's rate next to torch's fp64 product."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_ot import summary, windows  # noqa: E402

FP64_MATRIX_TFLOPS = 78.6
SHAPES = ((50000, 2048, 1000), (8192, 512, 256))


def sets(n, d, dev, seed=2024):
    g = torch.Generator(device=dev).manual_seed(seed + n + d)
    mix = (torch.eye(d, device=dev) + 0.5 * torch.randn(d, d, generator=g, device=dev) / (d ** 0.5)) / torch.sqrt(1.0 + torch.arange(d, device=dev))
    x = torch.randn(n, d, generator=g, device=dev) @ mix + 0.5
    y = (torch.randn(n, d, generator=g, device=dev) * 1.05) @ mix + 0.55
    return x.contiguous(), y.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frechet_moments_bench.json"))
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--old-windows", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frechet_moments: no GPU; timings are taken on the MI355X only")
    from flocoder_amd import distances as D
    from flocoder_amd import metrics as M
    dev = torch.device("cuda", 0)
    expectations, rows = {}, []

    for n, d, nb in SHAPES:
        x, y = sets(n, d, dev)
        batches = n // nb + (n % nb > 0)

        def feed(rows_):
            st = D.FrechetMoments()
            for r0 in range(0, n, nb):
                st.update(rows_[r0:r0 + nb])
            return st

        def old_stats(rows_):
            st = M.FrechetStatistics()
            for r0 in range(0, n, nb):
                st.update(rows_[r0:r0 + nb])
            return st

        a, b = feed(x), feed(y)
        fd, info = D.frechet_distance_moments(a, b, return_info=True)
        _, evals, factor_info = a.factor()
        cached_info = None

        def drop(*states):
            for st in states:
                st._factor = None

        def dist_cold(r):
            drop(a, b)
            return D.frechet_distance_moments(a, b)

        def dist_cached_real(r):
            drop(b)
            return D.frechet_distance_moments(a, b)

        def factor_only(r):
            drop(a)
            a.factor()

        def torch_gram(r):
            f = x[:nb].double()
            return f.t() @ f

        a.factor()
        drop(b)
        cached_info = D.frechet_distance_moments(a, b, return_info=True)[1]
        fns = {"update_pass": lambda r: feed(x), "existing_update_pass": lambda r: old_stats(x), "torch_fp64_gram": torch_gram,
               "factor": factor_only, "distance_nothing_cached": dist_cold, "distance_real_cached": dist_cached_real,
               "distance_both_cached": lambda r: D.frechet_distance_moments(a, b)}
        for fn in fns.values():
            fn(0)
        t = {name: summary(v) for name, v in windows(fns, args.windows, 1, dev).items()}
        so, sp = old_stats(x), old_stats(y)
        old_fns = {"existing_frechet_distance": lambda r: M.frechet_distance(*so.moments(), *sp.moments())}
        t.update({name: summary(v) for name, v in windows(old_fns, args.old_windows, 1, dev).items()})
        old_value = M.frechet_distance(*so.moments(), *sp.moments())

        per_batch = t["update_pass"]["median_ms"] / batches
        rate = nb * d * (d + 1.0) / (per_batch * 1e-3) / 1e12
        torch_rate = 2.0 * nb * d * d / (t["torch_fp64_gram"]["median_ms"] * 1e-3) / 1e12
        new_eval = {k: round(2.0 * t["update_pass"][k] + t["distance_nothing_cached"][k], 4) for k in ("median_ms", "min_ms", "max_ms")}
        old_eval = {k: round(2.0 * t["existing_update_pass"][k] + t["existing_frechet_distance"][k], 4) for k in ("median_ms", "min_ms", "max_ms")}
        row = {"n": n, "dim": d, "batch": nb, "batches_per_set": batches, **t,
               "update_per_batch_ms": round(per_batch, 4), "existing_update_per_batch_ms": round(t["existing_update_pass"]["median_ms"] / batches, 4),
               "update_tflops_lower_triangle": round(rate, 3), "update_fraction_of_fp64_matrix_peak": round(rate / FP64_MATRIX_TFLOPS, 4),
               "torch_fp64_gram_tflops_full_square": round(torch_rate, 3),
               "covariance_condition_number": float(evals[0] / evals[-1]), "sweeps": info["sweeps"], "launches_nothing_cached": info["launches"], "launches_real_cached": cached_info["launches"],
               "launches_factor": factor_info["launches"],
               "evaluation_ms": new_eval, "existing_evaluation_ms": old_eval,
               "existing_over_new": round(old_eval["median_ms"] / new_eval["median_ms"], 3),
               "value": fd, "existing_value": old_value, "value_minus_existing": fd - old_value}
        if d == 2048:
            expectations[f"(a) N = {n}, D = {d}: updates + distance faster than FrechetStatistics updates + frechet_distance"] = \
                new_eval["max_ms"] < old_eval["min_ms"]
        expectations[f"(b) N = {n}, D = {d}: the real side's cached factor saves one of three solves"] = \
            (cached_info["launches"] == info["launches"] - factor_info["launches"]
             and t["distance_real_cached"]["max_ms"] < t["distance_nothing_cached"]["min_ms"])
        expectations[f"(c) N = {n}, D = {d}: update rate next to torch's fp64 product (recorded, no requirement)"] = \
            f"recorded: {rate:.3f} TFLOP/s (lower triangle) against {torch_rate:.3f} TFLOP/s (full square)"
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, y, a, b, so, sp

    # ---- a set the sample form refuses, through fid_score
    g = torch.Generator(device=dev).manual_seed(7)
    real = torch.randn(20000, 1, 8, 8, generator=g, device=dev)
    fake = torch.randn(20000, 1, 8, 8, generator=g, device=dev) * 1.2 + 0.1

    def net(u8):
        return u8[:, 0].reshape(u8.shape[0], -1).float()

    kw = dict(device=dev, inception=net, chunk=True, chunk_size=1000)
    M.fid_score(real, fake, solver="moments", **kw)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    value = M.fid_score(real, fake, solver="moments", **kw)
    ms = 1e3 * (time.perf_counter() - t0)
    try:
        M.fid_score(real, fake, solver="jacobi", **kw)
        refused = False
    except ValueError:
        refused = True
    fid = {"images_per_side": 20000, "features": 64, "chunk_size": 1000, "moments_ms": round(ms, 3), "moments_value": value,
           "eig_value": M.fid_score(real, fake, solver="eig", **kw), "sample_form_refuses": refused}
    print(json.dumps(fid), flush=True)

    out = {"tool": "tools/bench_frechet_moments.py", "device": torch.cuda.get_device_name(dev),
           "timing": f"{args.windows} alternating windows ({args.old_windows} for the existing frechet_distance); host clock around device "
                     "synchronisations; median, min, max, spread = max - min over windows; one call per window; update_pass and "
                     "existing_update_pass are whole passes over one set; evaluation_ms = 2 update passes + the distance",
           "fp64_matrix_peak_tflops": {"value": FP64_MATRIX_TFLOPS, "source": "AMD Instinct MI355X data sheet, peak FP64 matrix; not measured here"},
           "expectations": {key: v if isinstance(v, str) else ("met" if v else "MISSED") for key, v in expectations.items()}, "shapes": rows, "fid_score": fid}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    missed = [key for key, v in expectations.items() if v is False]
    print(f"wrote {args.out}; expectations missed: {missed if missed else 'none'}")


if __name__ == "__main__":
    main()
