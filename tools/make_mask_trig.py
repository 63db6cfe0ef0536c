#!/usr/bin/env python3
"""Writes flocoder_amd/csrc/mask_trig.h, the step table of the inpainting masks' integer brush walk: MASK_TRIG[a] =
rint(0.7 * 65536 * cos(2 pi a / 4096)).  The file is committed; the device code includes it and flocoder_amd.noise parses it, so the two
sides hold the same numbers whatever either one's cosine returns.  Refuses to write if an entry sits within 1e-6 of a rounding tie (the
nearest is 2e-4 away), so that any fp64 cosine good to a few ulp reproduces the table (tests/test_masks_cpu.py)."""
import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flocoder_amd", "csrc", "mask_trig.h")
N = 4096
HEAD = """\
// The step table of the inpainting masks' integer brush walk (masks.hip; flocoder_amd/noise.py parses this file):
// MASK_TRIG[a] = rint(0.7 * 65536 * cos(2 pi a / 4096)), a step of 0.7 px in Q16; the sine is MASK_TRIG[(a - 1024) & 4095].
// Written by tools/make_mask_trig.py.  Both sides read these numbers; neither recomputes them.
#pragma once

#define FC_MASK_TRIG_BITS 12
__device__ const int MASK_TRIG[1 << FC_MASK_TRIG_BITS] = {
"""


def main():
    v = np.cos(np.arange(N, dtype=np.float64) * (2.0 * np.pi / N)) * (0.7 * 65536.0)
    tie = np.abs(np.abs(v - np.floor(v)) - 0.5).min()
    if tie < 1e-6:
        raise SystemExit(f"an entry is {tie:.3g} from a rounding tie")
    t = np.rint(v).astype(np.int64)
    rows = ["    " + ", ".join(str(int(x)) for x in t[i:i + 16]) for i in range(0, N, 16)]
    with open(OUT, "w") as f:
        f.write(HEAD + ",\n".join(rows) + "\n};\n")
    print(f"wrote {OUT}: min distance to a tie {tie:.3g}")


if __name__ == "__main__":
    main()
