#!/usr/bin/env python3
"""Pre-encoding's producer side, measured: the augmentation launch alone, the whole producer call, producer + ``VQVAE.encode`` at the
midi_vqgan.yaml shape against the same encode on a ready tensor, and the same PIL sequence on 16 host worker processes (when PIL can be
imported).  B = 64 and 256 at S = 128; the image form on a pool of synthetic 500 x 375 RGB sources, the MIDI form on 128 x 512 ones.

The expectation is the masks tool's: pre-encoding stays codec-bound -- producer + encode <= encode alone + the run-to-run spread of
encode alone measured in this session, the producer being ``AugmentedBatches`` as ``process_dataset`` walks it (the plain call +
encode, host table and launch in line, is reported beside it).  Prints met or MISSED per case and writes everything to ``profiles/augment_bench.json`` (``--out``).
The byte counts are reported against the 6.29 TB/s streaming figure, not gated."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_TBS = 6.29
SIZE, SEED, N_SOURCES, WORKERS = 128, 11, 64, 16


def image_source(k, h=375, w=500):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(x * 255 // (w - 1) + 5 * k) % 256, y * 255 // (h - 1), (x * y + k) % 256], axis=-1).astype(np.uint8)


def midi_source(k, h=128, w=512):
    rng = np.random.default_rng(k)
    return (rng.integers(0, 256, (h, w, 3)) * (rng.random((h, w, 3)) < 0.1)).astype(np.uint8)


def pil_worker(job):
    """One host worker: ``count`` variants as upstream makes them -- the file re-opened for each, rotate, centre crop, resized crop, flip,
    ToTensor + Normalize into fp32 -- with the definition's own draws."""
    from PIL import Image
    from flocoder_amd import noise as N
    path, first, count = job
    p = N.augment_image_params(SEED, np.arange(first, first + count), (375, 500), SIZE)
    t0 = time.perf_counter()
    for b in range(count):
        with Image.open(path) as im:
            im = im.convert("RGB")
            im = im.rotate(float(p["angle"][b]), Image.NEAREST, fillcolor=(0, 0, 0))
            t, l, s = int(p["crop_top"][b]), int(p["crop_left"][b]), int(p["crop_side"][b])
            im = im.crop((l, t, l + s, t + s))
            bx, by, bw, bh = (int(p[k][b]) for k in ("box_left", "box_top", "box_w", "box_h"))
            im = im.crop((bx, by, bx + bw, by + bh)).resize((SIZE, SIZE), Image.BILINEAR)
            if p["flip"][b]:
                im = im.transpose(Image.FLIP_LEFT_RIGHT)
            x = (np.asarray(im, dtype=np.float32).transpose(2, 0, 1) / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)
    assert x.shape == (3, SIZE, SIZE)
    return time.perf_counter() - t0


def pil_leg(per_worker=96):
    try:
        from PIL import Image
    except ImportError:
        return None
    import multiprocessing as mp
    with tempfile.TemporaryDirectory() as d:
        jobs = []
        for k in range(WORKERS):
            path = os.path.join(d, f"{k}.jpg")
            Image.fromarray(image_source(k)).save(path, quality=90)
            jobs.append((path, k * per_worker, per_worker))
        with mp.get_context("spawn").Pool(WORKERS) as pool:                 # started before this process touches the GPU; the workers never do
            pool.map(pil_worker, [(j[0], j[1], 4) for j in jobs])           # imports and first touches
            t0 = time.perf_counter()
            inner = pool.map(pil_worker, jobs)
            wall = time.perf_counter() - t0
    return {"workers": WORKERS, "variants": WORKERS * per_worker, "wall_s": round(wall, 3), "images_per_s": round(WORKERS * per_worker / wall, 1),
            "per_worker_images_per_s": round(per_worker / float(np.median(inner)), 1), "usable_cpus": len(os.sched_getaffinity(0))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    ap.add_argument("--no-pil", action="store_true")
    args = ap.parse_args()
    result = {"size": SIZE, "stream_tb_s": STREAM_TBS, "pil_host": None if args.no_pil else pil_leg()}
    print(json.dumps({"pil_host": result["pil_host"]}), flush=True)

    import torch
    from flocoder_amd import _binding as B
    from flocoder_amd import noise as N
    from flocoder_amd.augment import AugmentedBatches, ImagePool, augment_images, augment_midi
    from flocoder_amd.codecs import VQVAE
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    vq = VQVAE(in_channels=3, hidden_channels=256, num_downsamples=3, internal_dim=128, vq_embedding_dim=4, codebook_levels=4,
               vq_num_embeddings=96).eval().to(dev)
    pools = {"image": ImagePool.from_arrays([image_source(k) for k in range(N_SOURCES)], device=dev),
             "midi": ImagePool.from_arrays([midi_source(k) for k in range(N_SOURCES)], device=dev)}

    def gpu_ms(fn, reps):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
        return out

    def wall_ms(fn, reps):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0))
        return out

    result["cases"] = []
    for kind, pool in pools.items():
        for bsz in (64, 256):
            g = np.arange(bsz, dtype=np.int64)
            src, ids = g % len(pool), 1000 + g
            hw = pool.hw[src]
            stream = B.current_stream(dev)
            if kind == "image":
                p = N.augment_image_params(SEED, ids, hw, SIZE)
                stab = torch.from_numpy(N.augment_image_table(p, src, hw)).to(dev)
                out = torch.empty(bsz, 3, SIZE, SIZE, device=dev)
                half = (B.C.c_float * 3)(0.5, 0.5, 0.5)
                fill = (B.C.c_float * 3)(-1.0, -1.0, -1.0)
                launch = lambda: B.check(B.lib().fc_augment_images(B.ptr(out), B.ptr(pool.buffer), B.ptr(pool.table), len(pool), B.ptr(stab), bsz,
                                                                   SIZE, half, half, fill, stream))
                producer = lambda: augment_images(pool, src, ids, SIZE, SEED)
                read = int((p["box_w"] * p["box_h"]).sum() * 3 + stab.numel() * 4)     # the boxes' bytes, each once, and the table
            else:
                p = N.augment_midi_params(SEED, ids, hw, SIZE)
                stab = torch.from_numpy(N.augment_midi_table(p, src)).to(dev)
                out = torch.empty(bsz, 3, SIZE, SIZE, device=dev)
                launch = lambda: B.check(B.lib().fc_augment_midi(B.ptr(out), B.ptr(pool.buffer), B.ptr(pool.table), len(pool), B.ptr(stab), bsz,
                                                                 SIZE, 3, 0, 0.3, stream))
                producer = lambda: augment_midi(pool, src, ids, SIZE, SEED)
                read = int(bsz * SIZE * SIZE * 3 + stab.numel() * 4)
            write = bsz * 3 * SIZE * SIZE * 4
            t_launch = float(np.median(gpu_ms(launch, 20)))
            t_producer = float(np.median(wall_ms(producer, 20)))
            ready = producer()
            with torch.no_grad():
                enc = wall_ms(lambda: vq.encode(ready), 9)
                both = wall_ms(lambda: vq.encode(producer()), 9)
                # a control without any producer: the same encode on a copy made just before it (a fresh tensor, one device-side memcpy)
                fresh = wall_ms(lambda: vq.encode(ready.clone()), 9)
                # as process_dataset sees it: AugmentedBatches makes a batch's table beside the encode of the batch before
                loader = iter(AugmentedBatches(pool, 12 * bsz // len(pool), bsz, SIZE, seed=SEED, kind=kind))
                piped = wall_ms(lambda: vq.encode(next(loader)[0]), 9)
            t_enc, spread, t_both, t_piped = float(np.median(enc)), float(max(enc) - min(enc)), float(np.median(both)), float(np.median(piped))
            met = t_piped <= t_enc + spread
            case = {"kind": kind, "batch": bsz, "launch_ms": round(t_launch, 4), "launch_images_per_s": round(bsz / t_launch * 1e3, 1),
                    "read_bytes": read, "write_bytes": write, "launch_tb_s": round((read + write) / t_launch / 1e9, 3),
                    "frac_of_stream": round((read + write) / t_launch / 1e9 / STREAM_TBS, 4),
                    "producer_call_ms": round(t_producer, 4), "producer_images_per_s": round(bsz / t_producer * 1e3, 1),
                    "encode_ms": round(t_enc, 3), "encode_spread_ms": round(spread, 3), "encode_images_per_s": round(bsz / t_enc * 1e3, 1),
                    "producer_plus_encode_ms": round(t_both, 3), "loader_plus_encode_ms": round(t_piped, 3),
                    "copy_plus_encode_ms": round(float(np.median(fresh)), 3), "codec_bound": "met" if met else "MISSED"}
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
            print(f"{kind} B={bsz}: loader + encode {t_piped:.3f} ms (plain call + encode {t_both:.3f}, device copy + encode {float(np.median(fresh)):.3f}) against encode {t_enc:.3f} + spread {spread:.3f} ms: "
                  f"{'met' if met else 'MISSED'}",
                  flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
