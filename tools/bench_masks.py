#!/usr/bin/env python3
"""What the inpainting masks cost on the device, next to the NumPy form and next to the codec that consumes them.

    python tools/bench_masks.py [--batches 64 256 --reps 50 --windows 5 --host-masks 200 --out profiles/mask_bench.json]

Per batch size B at 128 x 128: masks/s of fc_inpaint_masks (through generate_mask_batch(unique_masks=True), i.e. with its two output
allocations and the sample ids made on the device) for every forced type and for the default mixture.  Once: masks/s of the NumPy form
flocoder_amd.noise.mask_field on this machine's host (one process), the CPU figure.  Per B: create_inpainting_triplet on a VQVAE of the
midi_vqgan.yaml shape (3 x 128 x 128 images, hidden 256, 3 downsamples) against its two codec.encode calls alone, on the same images.

Expectation, reported as met or MISSED: triplet production is codec-bound -- triplet <= encodes + the spread (max - min over the
windows) of the encodes' own time in this session: what the masks and the blend add is not told apart from the encodes' own variation."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_ot import summary, windows  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--codec-reps", type=int, default=4)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--host-masks", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_masks.py measures on an MI355X; no GPU found")
    from flocoder_amd import noise as N
    from flocoder_amd.codecs import VQVAE
    from flocoder_amd.inpainting import create_inpainting_triplet, generate_mask_batch
    device = torch.device("cuda", 0)
    size, seed = (128, 128), 2026
    kinds = ["mixture", *N.MASK_TYPES]

    host = {}
    for kind in kinds:
        ids = np.arange(args.host_masks)
        N.mask_field(seed, ids[:8], size, mask_type="" if kind == "mixture" else kind)
        t0 = time.perf_counter()
        N.mask_field(seed, ids, size, mask_type="" if kind == "mixture" else kind)
        host[kind] = round(args.host_masks / (time.perf_counter() - t0), 1)

    torch.manual_seed(0)
    codec = VQVAE(in_channels=3, hidden_channels=256, num_downsamples=3, internal_dim=128, vq_embedding_dim=4).eval().to(device)
    results = []
    for B in args.batches:
        fns = {}
        for kind in kinds:
            def fn(r, kind=kind):
                ids = torch.arange(r * B, (r + 1) * B, dtype=torch.int64, device=device)
                return generate_mask_batch(size, B, unique_masks=True, seed=seed, sample_ids=ids, device=device,
                                           mask_type="" if kind == "mixture" else kind)
            fn(0)
            fns[kind] = fn
        t = windows(fns, args.windows, args.reps, device)
        masks = {k: dict(summary(v), masks_per_s=round(B / (1e-3 * summary(v)["median_ms"]), 0)) for k, v in t.items()}

        images = torch.rand(B, 3, *size, generator=torch.Generator().manual_seed(B)).to(device)
        blank = images * 0.5

        def encodes(r):
            with torch.no_grad():
                return codec.encode(images), codec.encode(blank)

        def triplet(r):
            with torch.no_grad():
                return create_inpainting_triplet(images, codec, seed=seed, sample_ids=torch.arange(r * B, (r + 1) * B, dtype=torch.int64, device=device))
        encodes(0), triplet(0)
        tc = windows({"encodes": encodes, "triplet": triplet}, args.windows, args.codec_reps, device)
        e, tr = summary(tc["encodes"]), summary(tc["triplet"])
        allowed = e["median_ms"] + e["spread_ms"]
        row = {"batch": B, "size": list(size), "masks": masks, "two_encodes": e, "triplet": tr,
               "images_per_s_encode": round(2 * B / (1e-3 * e["median_ms"]), 0),
               "criterion": {"triplet_ms": tr["median_ms"], "allowed_ms": round(allowed, 4), "met": bool(tr["median_ms"] <= allowed)}}
        results.append(row)
        print(json.dumps(row), flush=True)
    met = all(r["criterion"]["met"] for r in results)
    doc = {"tool": "tools/bench_masks.py", "device": torch.cuda.get_device_name(device),
           "timing": f"{args.windows} alternating windows; {args.reps} mask calls / {args.codec_reps} codec calls per window; host clock around "
                     "device synchronisations; median, min, max, spread = max - min over windows; a mask call is generate_mask_batch("
                     "unique_masks=True): the ids (torch.arange on the device), two allocations, one launch",
           "codec": "VQVAE in_channels=3 hidden_channels=256 num_downsamples=3 internal_dim=128 (midi_vqgan.yaml), random weights, 3x128x128",
           "host_numpy_masks_per_s": dict(host, note=f"flocoder_amd.noise.mask_field, {args.host_masks} masks in one call, one process, "
                                                     "the host of the machine this ran on"),
           "expectations": {"triplet <= two encodes + the spread of the two encodes (codec-bound)": "met" if met else "MISSED"},
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}; codec-bound expectation {'met' if met else 'MISSED'}")


if __name__ == "__main__":
    main()
