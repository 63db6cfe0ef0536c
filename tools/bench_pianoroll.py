#!/usr/bin/env python3
"""What decoding piano-roll images to notes costs on the device, next to the NumPy definition on the host, and sampler + decoder next to
their parts.

    python tools/bench_pianoroll.py [--batches 64 256 --reps 10 --windows 5 --steps 10 --out profiles/pianoroll_bench.json]

* images_to_notes at B x 3 x 128 x 128 (painted by notes_to_images from random note lists) and on one 2048 x 2048 grid: the launches
  alone between two device events (``max_notes=n``: nothing waits), the whole call (``max_notes=None``: the counts are read once), and
  ``images_to_notes_np`` on the host (timed on ``--host-images`` images and scaled to the batch; the grid in full).
* sampler(..., is_midi=True) followed by images_to_notes on what it returns, against the two timed separately.

Expectations, each reported as met or MISSED: the whole call is faster than the definition on the host; sampler + images_to_notes costs
no more than its parts plus the spread (max - min over the windows) measured on them."""
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

from bench_eval import device_time_ms  # noqa: E402
from bench_ot import summary, windows  # noqa: E402


def random_rolls(batch, width, per_roll, seed, device):
    """uint8 [batch,3,128,width]: `per_roll` random notes per roll, painted on the device."""
    from flocoder_amd import pianoroll as P
    rng = np.random.default_rng(seed)
    start = rng.integers(0, width - 1, size=(batch, per_roll))
    notes = np.stack([rng.integers(1, 127, size=(batch, per_roll)), start, start + rng.integers(1, 24, size=(batch, per_roll)),
                      rng.integers(11, 128, size=(batch, per_roll))], axis=2).astype(np.int32)
    counts = torch.full((batch,), per_roll, dtype=torch.int64, device=device)
    return P.notes_to_images(torch.from_numpy(notes).to(device), counts, width)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--host-images", type=int, default=8)
    ap.add_argument("--sample-batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pianoroll_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pianoroll.py measures on an MI355X; no GPU found")
    from flocoder_amd import pianoroll as P
    from flocoder_amd import sampling as S
    from flocoder_amd.codecs import VQVAE
    from flocoder_amd.unet import Unet
    device = torch.device("cuda", 0)
    expectations, rows = {}, []

    cases = [(f"B={b} 128x128", random_rolls(b, 128, 60, b, device), args.host_images) for b in args.batches]
    strips = random_rolls(16, 2048, 900, 7, device)                              # 16 strips of 2048 columns stacked: one 2048 x 2048 image
    cases.append(("grid 2048x2048", strips.permute(1, 0, 2, 3).reshape(1, 3, 2048, 2048).contiguous(), 1))
    for name, images, host_n in cases:
        notes, counts = P.images_to_notes(images)
        n = notes.shape[1]
        host = images[:host_n].cpu().numpy()
        t0 = time.perf_counter()
        want, want_counts = P.images_to_notes_np(host)
        host_ms = 1e3 * (time.perf_counter() - t0) * images.shape[0] / host_n
        assert np.array_equal(want_counts, counts[:host_n].cpu().numpy())
        assert np.array_equal(want, notes[:host_n, :want.shape[1]].cpu().numpy())
        t = windows({"whole_call": lambda r: P.images_to_notes(images), "no_wait_call": lambda r: P.images_to_notes(images, max_notes=n)},
                    args.windows, args.reps, device)
        dev_ms = device_time_ms(lambda: P.images_to_notes(images, max_notes=n), 100, device)
        row = {"case": name, "shape": list(images.shape), "notes_per_roll_max": n, "notes_total": int(counts.sum()),
               **{k: summary(v) for k, v in t.items()},
               "launches_alone": {"ms": round(dev_ms, 5), "what": "scan (3 launches) + memset + emit, 100 calls between two device events"},
               "numpy_definition_host_ms": round(host_ms, 2), "host_images_timed": host_n}
        expectations[f"images_to_notes {name} faster than the definition on the host"] = row["whole_call"]["median_ms"] < host_ms
        rows.append(row)
        print(json.dumps(row), flush=True)

    # ---- sampler + images_to_notes against the parts
    B, levels, size = args.sample_batch, 4, 512
    torch.manual_seed(0)
    model = Unet(dim=32, dim_mults=(1, 2, 4, 8), channels=4, n_classes=0).to(device).eval()
    codec = VQVAE(in_channels=3, hidden_channels=256, num_downsamples=3, internal_dim=128, vq_embedding_dim=4, vq_num_embeddings=size,
                  codebook_levels=levels).eval()
    g = torch.Generator().manual_seed(5)
    for i in range(levels):
        codec.vq.layers[i]._codebook.embed.copy_(torch.randn(1, size, 4, generator=g) * (0.5 ** i))
        codec.vq.layers[i]._codebook.initted.fill_(True)
    codec = codec.to(device)
    source = torch.randn(B, 4, 16, 16, generator=g).to(device)
    kw = dict(method="rk4", batch_size=B, n_steps=args.steps, n_classes=0, latent_shape=(4, 16, 16), is_midi=True, source=source)
    decoded = S.sampler(model, codec, **kw)[1]
    parts = {"sampler": lambda r: S.sampler(model, codec, **kw), "images_to_notes": lambda r: P.images_to_notes(decoded, require_onsets=False)}

    def both(r):
        return P.images_to_notes(S.sampler(model, codec, **kw)[1], require_onsets=False)
    both(0)
    s = {k: summary(v) for k, v in windows({"sampler_then_notes": both, **parts}, args.windows, max(2, args.reps // 3), device).items()}
    parts_ms = sum(s[k]["median_ms"] for k in parts)
    allowed = parts_ms + sum(s[k]["spread_ms"] for k in parts)
    comp = {"batch": B, "rk4_steps": args.steps, "decoded": list(decoded.shape), "dtype": str(decoded.dtype), **s,
            "sum_of_parts_ms": round(parts_ms, 4), "allowed_ms": round(allowed, 4)}
    expectations["sampler + images_to_notes <= its parts + the spread measured on the parts"] = s["sampler_then_notes"]["median_ms"] <= allowed
    print(json.dumps(comp), flush=True)

    doc = {"tool": "tools/bench_pianoroll.py", "device": torch.cuda.get_device_name(device),
           "timing": f"{args.windows} alternating windows; host clock around device synchronisations; median, min, max, spread = max - min over "
                     f"windows; {args.reps} decoder calls, {max(2, args.reps // 3)} sampler calls per window",
           "expectations": {k: "met" if v else "MISSED" for k, v in expectations.items()}, "images_to_notes": rows, "sampler_and_notes": comp}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    missed = [k for k, v in expectations.items() if not v]
    print(f"wrote {args.out}; expectations missed: {missed if missed else 'none'}")


if __name__ == "__main__":
    main()
