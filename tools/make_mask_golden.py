#!/usr/bin/env python3
"""tests/golden/g13_masks.npz: what the *reference's* mask generator (flocoder/inpainting.py generate_mask, run from the read-only
reference tree, never copied) draws, as recorded results only -- the yardstick of the counter-based restatement in
``flocoder_amd.noise.mask_field`` (tests/test_masks_cpu.py).

Under ``np.random.seed(SEED)`` and in the order of ``TYPES``, N masks of every type at 128 x 128 with the type forced.  Stored:

    types      the type names, in order
    coverage   uint16 [3, N]         number of set pixels of every mask (coverage fraction = coverage / 16384)
    counts     uint16 [3, 128, 128]  how many of the N masks set each pixel (per-pixel mean image = counts / N)
    n, seed    N and the NumPy seed

Runs in the build container only (``python tools/make_mask_golden.py``, about two minutes of one core).
"""
import importlib.util
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("FLOCODER_REFERENCE", "/root/reference")
OUT = os.path.join(REPO, "tests", "golden", "g13_masks.npz")
TYPES = ("brush", "rectangles", "noise")
N, SEED, SIZE = 4000, 20261019, (128, 128)


def import_reference_inpainting():
    spec = importlib.util.spec_from_file_location("ref_inpainting", os.path.join(REF, "flocoder", "inpainting.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod._status_msg = "quiet"          # the one-time banner of generate_mask
    return mod


def main():
    ref = import_reference_inpainting()
    np.random.seed(SEED)
    coverage = np.zeros((len(TYPES), N), dtype=np.uint16)
    counts = np.zeros((len(TYPES), *SIZE), dtype=np.uint16)
    for k, name in enumerate(TYPES):
        for i in range(N):
            m = np.asarray(ref.generate_mask(size=SIZE, mask_type=name, to_tensor=False)) != 0
            assert m.shape == SIZE
            coverage[k, i] = m.sum()
            counts[k] += m
        print(f"{name}: mean coverage {coverage[k].mean() / m.size:.4f}")
    np.savez_compressed(OUT, types=np.array(TYPES), coverage=coverage, counts=counts, n=np.int64(N), seed=np.int64(SEED))
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
