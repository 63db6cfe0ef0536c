#!/usr/bin/env python3
"""Exact k-NN and PRDC on the device, measured (flocoder_amd.neighbors, metrics.prdc; csrc/knn.hip).

    python tools/bench_knn.py [--windows 5 --reps 5 --out profiles/knn_bench.json]

All shapes are 4 x 32 x 32 latents (D = 4096), Gaussian, with the references resident on the device:

* ``knn`` at Q = 64 against N = 16,384 and 65,536 at k = 1, 5 and 64;
* ``knn`` (self, query_ids) and ``ball_counts`` at Q = N = 8192, k = 5 -- PRDC's calls -- and ``prdc`` itself at that shape (the fake
  set is a Gaussian 5 % wider and shifted by 0.05: in 4096 dimensions none of it falls into a real ball, so the recorded values are
  precision, density and coverage 0 and recall 1 -- they are there for the record, the shape is there for the time);
* for context ``torch.cdist(q, r).topk(k, largest=False)`` on the same tensors (the GEMM form, which materialises Q x N distances);
* validity on a data set with planted near-duplicates (Q = 64 queries, N = 8192 references, eight references per query at squared
  distances 1e-4 (1 + m / 100), m = 0..7): a query's answer counts as valid when no reference outside its index set is closer than one
  inside it by more than the derived bound e(D) allows, judged on fp64 direct differences.  Counted for both forms;
* ``evaluate_model`` with and without ``prdc_k=5`` on the models of tools/bench_eval.py, and ``prdc`` alone on the same latents;
* one ``nearest_in_dataset`` run over a packed file of ``--dataset-rows`` latents in a temporary directory, next to the device time
  of the same updates on resident chunks: the kernel's share of the run.

Per shape: time per call, the achieved fraction of the fp32 vector peak at 3 operations per pair-element (subtract, multiply, add:
157.3 TFLOP/s, MI355X_MICROARCH.md) and of the streaming figure (6.29 TB/s measured, float4 copy) for the reference bytes read once.
Every sample is the host time of ``reps`` calls ending in a device synchronise; the sides alternate window by window; medians and the
spread (max - min over the windows) are reported.

Expectations, each reported as met or MISSED:
(a) evaluate_model(prdc_k=5) costs no more than evaluate_model() plus prdc timed alone, plus the spread measured on evaluate_model();
(b) knn time grows no faster than linearly from N = 16,384 to 65,536 at fixed Q: the slowest window at 65,536 is at most four times
    the median at 16,384 plus its spread."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_ot import summary, windows  # noqa: E402

VALU_TFLOPS, STREAM_TBS, DIM = 157.3, 6.29, 4096


def rates(ms, nq, n, calls=1):
    """Fractions of the two ceilings for `calls` passes over nq x n pairs in `ms`."""
    sec = ms * 1e-3
    return {"valu_fraction": round(3.0 * nq * n * DIM * calls / sec / (VALU_TFLOPS * 1e12), 4),
            "stream_fraction": round(4.0 * n * DIM * calls / sec / (STREAM_TBS * 1e12), 4)}


def error_bound(dim):
    """e(D) = (D + 2) u / (1 - (D + 2) u), u = 2^-24: the relative bound on an fp32 d2 of D features."""
    u = 2.0 ** -24
    return (dim + 2) * u / (1.0 - (dim + 2) * u)


def exact_d2(q, r, chunk=512):
    """fp64 direct differences on the device, [Q, N]."""
    q64 = q.double()
    return torch.cat([(q64[:, None, :] - r[lo:lo + chunk].double()[None]).square().sum(-1) for lo in range(0, r.shape[0], chunk)], dim=1)


def invalid_queries(idx, d2, e):
    """Queries whose index set is not a k-NN set under the bound: some reference outside it lies closer than one inside it by more than
    rounding explains, max_in d (1 - e) > min_out d (1 + e)."""
    inside = torch.zeros_like(d2, dtype=torch.bool).scatter_(1, idx, True)
    worst_in = torch.where(inside, d2, torch.zeros_like(d2)).amax(dim=1)
    best_out = torch.where(inside, torch.full_like(d2, float("inf")), d2).amin(dim=1)
    return int((worst_in * (1 - e) > best_out * (1 + e)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_bench.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dataset-rows", type=int, default=65536)
    ap.add_argument("--eval-batch", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn: no GPU; timings are taken on the MI355X only")
    from flocoder_amd import metrics as M
    from flocoder_amd import neighbors as NB
    from flocoder_amd import sampling as S
    from flocoder_amd.codecs import VQVAE
    from flocoder_amd.data import PackedLatentDataset, pack_latents
    from flocoder_amd.unet import Unet
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(2024)
    expectations, doc = {}, {}

    # ---- knn at Q = 64
    q = torch.randn(64, 4, 32, 32, generator=g).to(dev)
    refs = torch.randn(65536, 4, 32, 32, generator=g).to(dev)
    qf, rf = q.reshape(64, -1), refs.reshape(65536, -1)
    fns = {}
    for n in (16384, 65536):
        for k in (1, 5, 64):
            fns[f"knn_N{n}_k{k}"] = lambda r, n=n, k=k: NB.knn(q, refs[:n], k)
            fns[f"torch_cdist_topk_N{n}_k{k}"] = lambda r, n=n, k=k: torch.cdist(qf, rf[:n]).topk(k, largest=False)
    for fn in fns.values():
        fn(0)
    t = {name: summary(v) for name, v in windows(fns, args.windows, args.reps, dev).items()}
    rows = []
    for k in (1, 5, 64):
        small, big = t[f"knn_N16384_k{k}"], t[f"knn_N65536_k{k}"]
        met = big["max_ms"] <= 4 * small["median_ms"] + small["spread_ms"]
        expectations[f"(b) knn k={k}: N = 65536 within four times N = 16384"] = met
        for n in (16384, 65536):
            ours, tor = t[f"knn_N{n}_k{k}"], t[f"torch_cdist_topk_N{n}_k{k}"]
            rows.append({"queries": 64, "refs": n, "k": k, "knn": ours, **rates(ours["median_ms"], 64, n), "torch_cdist_topk": tor,
                         "torch_over_knn": round(tor["median_ms"] / ours["median_ms"], 3)})
            print(json.dumps(rows[-1]), flush=True)
    doc["knn_q64"] = rows
    del refs, rf

    # ---- PRDC's shape
    n, k = 8192, 5
    real = torch.randn(n, 4, 32, 32, generator=g).to(dev)
    fake = (torch.randn(n, 4, 32, 32, generator=g) * 1.05 + 0.05).to(dev)
    ids = torch.arange(n, device=dev)
    radius = NB.knn(real, real, k, query_ids=ids)[0][:, k - 1].contiguous()
    ff, rr = fake.reshape(n, -1), real.reshape(n, -1)
    fns = {"knn_self": lambda r: NB.knn(real, real, k, query_ids=ids), "ball_counts": lambda r: NB.ball_counts(fake, real, radius),
           "knn_cross_k1": lambda r: NB.knn(real, fake, 1), "prdc": lambda r: M.prdc(real, fake, k),
           "torch_cdist_topk": lambda r: torch.cdist(rr, rr).topk(k + 1, largest=False),
           "torch_cdist_count": lambda r: (torch.cdist(ff, rr).square() <= radius[None, :]).sum(dim=1)}
    for fn in fns.values():
        fn(0)
    t = {name: summary(v) for name, v in windows(fns, args.windows, max(1, args.reps // 2), dev).items()}
    row = {"real": n, "fake": n, "k": k, **t, "values": M.prdc(real, fake, k),
           "knn_self_rates": rates(t["knn_self"]["median_ms"], n, n), "ball_counts_rates": rates(t["ball_counts"]["median_ms"], n, n),
           "prdc_rates": rates(t["prdc"]["median_ms"], n, n, calls=5),
           "torch_over_knn_self": round(t["torch_cdist_topk"]["median_ms"] / t["knn_self"]["median_ms"], 3)}
    print(json.dumps(row), flush=True)
    doc["prdc_shape"] = row
    del real, fake, ff, rr

    # ---- planted near-duplicates: whose answer is a k-NN set?
    nq, n = 64, 8192
    q = torch.randn(nq, DIM, generator=g)
    refs = torch.randn(n, DIM, generator=g)
    for i in range(nq):
        for m in range(8):
            u = torch.randn(DIM, generator=g)
            refs[i * 8 + m] = q[i] + u / u.norm() * (1e-4 * (1 + m / 100.0)) ** 0.5
    q, refs = q.to(dev), refs.to(dev)
    d2, e = exact_d2(q, refs), error_bound(DIM)
    planted = {"queries": nq, "refs": n, "dim": DIM, "planted_per_query": 8, "planted_d2": "1e-4 (1 + m / 100), m = 0..7", "bound_e": e, "k": {}}
    for k in (1, 5, 64):
        planted["k"][str(k)] = {"knn_invalid_queries": invalid_queries(NB.knn(q, refs, k)[1], d2, e),
                                "torch_cdist_topk_invalid_queries": invalid_queries(torch.cdist(q, refs).topk(k, largest=False)[1], d2, e)}
    near = torch.cdist(q, refs).square()[torch.arange(nq, device=dev), 8 * torch.arange(nq, device=dev)]
    planted["torch_cdist_d2_of_the_nearest_planted"] = {"exact": 1e-4, "min": float(near.min()), "max": float(near.max())}
    ours = NB.knn(q, refs, 1)[0][:, 0]
    planted["knn_d2_of_the_nearest_planted"] = {"exact": 1e-4, "min": float(ours.min()), "max": float(ours.max())}
    print(json.dumps(planted), flush=True)
    doc["planted_near_duplicates"] = planted
    del q, refs, d2

    # ---- (a) evaluate_model with prdc_k
    B, levels, size = args.eval_batch, 4, 512
    torch.manual_seed(0)
    model = Unet(dim=32, dim_mults=(1, 2, 4, 8), channels=4, n_classes=0).to(dev)
    codec = VQVAE(in_channels=3, hidden_channels=256, num_downsamples=3, internal_dim=128, vq_embedding_dim=4, vq_num_embeddings=size,
                  codebook_levels=levels).eval()
    for i in range(levels):
        codec.vq.layers[i]._codebook.embed.copy_(torch.randn(1, size, 4, generator=g) * (0.5 ** i))
        codec.vq.layers[i]._codebook.initted.fill_(True)
    codec = codec.to(dev)
    target = torch.randn(B, 4, 16, 16, generator=g).to(dev)
    source = torch.randn(B, 4, 16, 16, generator=g).to(dev)
    kw = dict(batch_size=B, n_steps=10, is_midi=True, source=source)
    _, images = S.evaluate_model(model, codec, 0, target, return_images=True, **kw)
    pred = images["pred_latents"]
    fns = {"evaluate_model": lambda r: S.evaluate_model(model, codec, 0, target, **kw),
           "evaluate_model_prdc_k5": lambda r: S.evaluate_model(model, codec, 0, target, prdc_k=5, **kw),
           "prdc_alone": lambda r: M.prdc(target, pred, 5)}
    for fn in fns.values():
        fn(0)
    t = {name: summary(v) for name, v in windows(fns, args.windows, 2, dev).items()}
    allowed = t["evaluate_model"]["median_ms"] + t["prdc_alone"]["median_ms"] + t["evaluate_model"]["spread_ms"]
    expectations["(a) evaluate_model(prdc_k=5) <= evaluate_model() + prdc alone + the spread of evaluate_model()"] = \
        t["evaluate_model_prdc_k5"]["median_ms"] <= allowed
    doc["evaluate_model"] = {"batch": B, "latents": "4 x 16 x 16", "rk4_steps": 10, **t, "allowed_ms": round(allowed, 4)}
    print(json.dumps(doc["evaluate_model"]), flush=True)
    model.eval()

    # ---- nearest_in_dataset over a packed file: one run, and the kernel's share of it
    rows_n, chunk_rows = args.dataset_rows, 8192
    q = torch.randn(64, 4, 32, 32, generator=g).to(dev)
    with tempfile.TemporaryDirectory() as tmp:
        data = torch.from_numpy(np.random.default_rng(7).standard_normal((rows_n, 4, 32, 32), dtype=np.float32))

        class Items(torch.utils.data.Dataset):
            def __len__(self):
                return rows_n

            def __getitem__(self, i):
                return data[i], 0

        path = os.path.join(tmp, "latents.pack")
        pack_latents(Items(), path)
        ds = PackedLatentDataset(path)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        d_file, i_file = NB.nearest_in_dataset(q, ds, k=5, chunk_rows=chunk_rows)
        torch.cuda.synchronize(dev)
        run_ms = 1e3 * (time.perf_counter() - t0)
        resident = data[:chunk_rows].to(dev)

        def updates(r):
            search = NB.KnnSearch(q, 5)
            for lo in range(0, rows_n, chunk_rows):
                search.update(resident[:min(chunk_rows, rows_n - lo)], first_index=lo)
        updates(0)
        kern = summary(windows({"updates": updates}, args.windows, 2, dev)["updates"])
        whole = NB.knn(q, data.to(dev), 5)
        doc["nearest_in_dataset"] = {"rows": rows_n, "chunk_rows": chunk_rows, "queries": 64, "k": 5, "file_bytes": os.path.getsize(path),
                                     "one_run_ms": round(run_ms, 2), "updates_on_resident_chunks": kern,
                                     "kernel_share_of_the_run": round(kern["median_ms"] / run_ms, 4),
                                     "equals_knn_on_resident_rows": bool(torch.equal(d_file, whole[0]) and torch.equal(i_file, whole[1]))}
    print(json.dumps(doc["nearest_in_dataset"]), flush=True)

    out = {"tool": "tools/bench_knn.py", "device": torch.cuda.get_device_name(dev),
           "timing": f"{args.windows} alternating windows; host clock around device synchronisations; median, min, max, spread = max - min over "
                     f"windows; {args.reps} calls per window at Q = 64, {max(1, args.reps // 2)} at PRDC's shape, 2 evaluations",
           "ceilings": {"fp32_vector_tflops": VALU_TFLOPS, "stream_tb_per_s": STREAM_TBS, "operations_per_pair_element": 3},
           "expectations": {key: "met" if v else "MISSED" for key, v in expectations.items()}, **doc}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    missed = [key for key, v in expectations.items() if not v]
    print(f"wrote {args.out}; expectations missed: {missed if missed else 'none'}")


if __name__ == "__main__":
    main()
