#!/usr/bin/env python3
"""Frechet and kernel distances between sample sets on the device, measured (flocoder_amd.distances; csrc/frechet.hip).

    python tools/bench_frechet.py [--windows 3 --out profiles/frechet_bench.json --old-4096-limit-s 150]

Gaussian sets of N samples each in D dimensions, resident on the device, at (N, D) = (256, 4096), (2048, 1024), (2048, 4096) and
(256, 49152):

* ``frechet_distance_sets`` and ``kernel_distance``, whole calls (each ends in the host's read of the result);
* the Frechet call split into its Gram (``fc_gram_f64`` alone on precomputed means), its Jacobi solve (``singular_values`` of that
  Gram, including the copy of the matrix that call makes) and the rest (total minus the two: moments, the final sums, allocation, the
  read), with the sweeps and the number of kernel launches of the call;
* the Gram's rate in TFLOP/s at 2 N1 N2 D operations, and as a fraction of the 78.6 TFLOP/s peak fp64 matrix rate AMD's MI355X data
  sheet states (the rate is a vendor figure, not one measured here);
* the existing path, ``metrics.FrechetStatistics`` + ``metrics.frechet_distance`` (two D x D covariances on the device, their product to
  the host, a non-symmetric ``eigvals`` on the CPU) on the same inputs where D <= 2048; at (256, 4096) one sample of it in a child
  process with a time limit (``--old-4096-limit-s``; 0 skips it), reported as not finished when the limit ends it;
* ``evaluate_model`` with and without ``frechet=True, kid=True`` on the models of tools/bench_eval.py, and the four distance calls alone
  on the same tensors.

Every sample is the host time of ``reps`` calls ending in a device synchronise; the sides alternate window by window; medians and the
spread (max - min over the windows) are reported.

Expectations, each reported as met or MISSED:
(a) the new path is faster than the existing one at every shape where both ran (slowest window of the new against the fastest of the old);
(b) evaluate_model(frechet=True, kid=True) costs no more than evaluate_model() plus the four calls timed alone, plus the spread measured
    on evaluate_model()."""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_ot import summary, windows  # noqa: E402

FP64_MATRIX_TFLOPS = 78.6
SHAPES = ((256, 4096), (2048, 1024), (2048, 4096), (256, 49152))


def sets(n, d, dev, seed=2024):
    g = torch.Generator().manual_seed(seed + n + d)
    return torch.randn(n, d, generator=g).to(dev), (torch.randn(n, d, generator=g) * 1.05 + 0.05).to(dev)


def old_path(x, y):
    from flocoder_amd import metrics as M
    stats = (M.FrechetStatistics(), M.FrechetStatistics())
    stats[0].update(x)
    stats[1].update(y)
    return M.frechet_distance(*stats[0].moments(), *stats[1].moments())


def old_path_once(n, d):
    """Child mode: one timed sample of the existing path, printed as JSON."""
    dev = torch.device("cuda", 0)
    x, y = sets(n, d, dev)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    value = old_path(x, y)
    print(json.dumps({"ms": round(1e3 * (time.perf_counter() - t0), 1), "value": value}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frechet_bench.json"))
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--eval-batch", type=int, default=256)
    ap.add_argument("--old-4096-limit-s", type=float, default=150.0)
    ap.add_argument("--old-once", type=int, nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frechet: no GPU; timings are taken on the MI355X only")
    if args.old_once:
        return old_path_once(*args.old_once)
    from flocoder_amd import _binding as B
    from flocoder_amd import distances as D
    from flocoder_amd import sampling as S
    from flocoder_amd.codecs import VQVAE
    from flocoder_amd.unet import Unet
    dev = torch.device("cuda", 0)
    expectations, rows = {}, []

    for n, d in SHAPES:
        x, y = sets(n, d, dev)
        fd, info = D.frechet_distance_sets(x, y, return_info=True)
        mx, my = D._moments(x)[0], D._moments(y)[0]
        c = torch.empty(n, n, dtype=torch.float64, device=dev)
        scale = 1.0 / (n - 1.0)

        def gram_only(r):
            B.check(B.lib().fc_gram_f64(B.ptr(x), n, B.ptr(y), n, d, B.ptr(mx), B.ptr(my), scale, B.ptr(c), None, None, B.current_stream(dev)))
        gram_only(0)
        fns = {"frechet": lambda r: D.frechet_distance_sets(x, y), "kid": lambda r: D.kernel_distance(x, y), "gram": gram_only,
               "jacobi": lambda r: D.singular_values(c)}
        old = d <= 2048
        if old:
            fns["existing_path"] = lambda r: old_path(x, y)
        reps = 3 if n <= 256 else 1
        t = {name: summary(v) for name, v in windows(fns, args.windows, reps, dev).items()}
        tflops = 2.0 * n * n * d / (t["gram"]["median_ms"] * 1e-3) / 1e12
        row = {"n": n, "dim": d, "frechet": t["frechet"], "kid": t["kid"], "value": fd, "kid_value": D.kernel_distance(x, y),
               "sweeps": info["sweeps"], "launches": info["launches"],
               "split_ms": {"gram": t["gram"]["median_ms"], "jacobi": t["jacobi"]["median_ms"],
                            "rest": round(t["frechet"]["median_ms"] - t["gram"]["median_ms"] - t["jacobi"]["median_ms"], 4)},
               "gram_tflops": round(tflops, 3), "gram_fraction_of_fp64_matrix_peak": round(tflops / FP64_MATRIX_TFLOPS, 4)}
        if old:
            row["existing_path"] = t["existing_path"]
            row["existing_value"] = old_path(x, y)
            row["existing_over_new"] = round(t["existing_path"]["median_ms"] / t["frechet"]["median_ms"], 3)
            expectations[f"(a) N = {n}, D = {d}: frechet_distance_sets faster than FrechetStatistics + frechet_distance"] = \
                t["frechet"]["max_ms"] < t["existing_path"]["min_ms"]
        elif d == 4096 and n == 256 and args.old_4096_limit_s > 0:
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--old-once", str(n), str(d)], capture_output=True, text=True,
                                   timeout=args.old_4096_limit_s)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
                row["existing_path_one_sample"] = json.loads(line[-1]) if r.returncode == 0 and line else {"failed": r.returncode}
                if "ms" in row["existing_path_one_sample"]:
                    expectations[f"(a) N = {n}, D = {d}: frechet_distance_sets faster than one sample of the existing path"] = \
                        t["frechet"]["max_ms"] < row["existing_path_one_sample"]["ms"]
            except subprocess.TimeoutExpired:
                row["existing_path_one_sample"] = {"not_finished_within_s": args.old_4096_limit_s}
        else:
            row["existing_path"] = "not run: two D x D fp64 covariances and a CPU eigvals of that size"
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, y, c

    # ---- (b) evaluate_model with the two flags
    bsz, levels, size = args.eval_batch, 4, 512
    g = torch.Generator().manual_seed(2024)
    torch.manual_seed(0)
    model = Unet(dim=32, dim_mults=(1, 2, 4, 8), channels=4, n_classes=0).to(dev)
    codec = VQVAE(in_channels=3, hidden_channels=256, num_downsamples=3, internal_dim=128, vq_embedding_dim=4, vq_num_embeddings=size,
                  codebook_levels=levels).eval()
    for i in range(levels):
        codec.vq.layers[i]._codebook.embed.copy_(torch.randn(1, size, 4, generator=g) * (0.5 ** i))
        codec.vq.layers[i]._codebook.initted.fill_(True)
    codec = codec.to(dev)
    target = torch.randn(bsz, 4, 16, 16, generator=g).to(dev)
    source = torch.randn(bsz, 4, 16, 16, generator=g).to(dev)
    kw = dict(batch_size=bsz, n_steps=10, is_midi=True, source=source)
    _, im = S.evaluate_model(model, codec, 0, target, return_images=True, **kw)

    def four_calls(r):
        for fn in (D.frechet_distance_sets, D.kernel_distance):
            fn(target, im["pred_latents"])
            fn(im["decoded_target"], im["decoded_pred"])
    fns = {"evaluate_model": lambda r: S.evaluate_model(model, codec, 0, target, **kw),
           "evaluate_model_frechet_kid": lambda r: S.evaluate_model(model, codec, 0, target, frechet=True, kid=True, **kw),
           "four_calls_alone": four_calls}
    for fn in fns.values():
        fn(0)
    t = {name: summary(v) for name, v in windows(fns, max(args.windows, 5), 2, dev).items()}
    allowed = t["evaluate_model"]["median_ms"] + t["four_calls_alone"]["median_ms"] + t["evaluate_model"]["spread_ms"]
    expectations["(b) evaluate_model(frechet=True, kid=True) <= evaluate_model() + the four calls alone + the spread of evaluate_model()"] = \
        t["evaluate_model_frechet_kid"]["median_ms"] <= allowed
    ev = {"batch": bsz, "latents": "4 x 16 x 16", "pixels": "x".join(str(v) for v in im["decoded_pred"].shape[1:]), "rk4_steps": 10, **t,
          "allowed_ms": round(allowed, 4)}
    print(json.dumps(ev), flush=True)
    model.eval()

    out = {"tool": "tools/bench_frechet.py", "device": torch.cuda.get_device_name(dev),
           "timing": f"{args.windows} alternating windows ({max(args.windows, 5)} for evaluate_model); host clock around device synchronisations; "
                     "median, min, max, spread = max - min over windows; 3 calls per window at N = 256, 1 at N = 2048, 2 evaluations",
           "fp64_matrix_peak_tflops": {"value": FP64_MATRIX_TFLOPS, "source": "AMD Instinct MI355X data sheet, peak FP64 matrix; not measured here"},
           "expectations": {key: "met" if v else "MISSED" for key, v in expectations.items()}, "shapes": rows, "evaluate_model": ev}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    missed = [key for key, v in expectations.items() if not v]
    print(f"wrote {args.out}; expectations missed: {missed if missed else 'none'}")


if __name__ == "__main__":
    main()
