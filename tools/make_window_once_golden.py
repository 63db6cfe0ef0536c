#!/usr/bin/env python3
"""tests/golden/window_once_parent.npz: forwards of the dim-32 U-Net at 4x32x32, recorded ON THE BUILD BEFORE the register-fed Block-closing
convolutions staged their whole input window in the prologue (conv_dev.h FL_WW), for tests/test_gpu_conv_window_once.py to compare bit
for bit.

    python tools/make_window_once_golden.py [out.npz]            (needs the GPU; run it on a checkout of the commit to compare with)

Weights and inputs are the synthetic ones of the other goldens (oracle/synth.py: a function of name, shape and seed only).  Two plans:
one built for 64 rows and run at B = 1 and B = 3 (the two-sample tiles of the 4x4 level then hold an empty second sample, and an odd last
pair), and one built for 3 rows, whose small grids put more of the Block closes on the 32-row tile.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.synth import synth_input, synth_state_dict  # noqa: E402

SEED = 23
H = W = 32
CASES = ((64, 1), (64, 3), (3, 3))        # (rows the plan is built for, B)


def state_dict():
    from conftest import load_golden
    return synth_state_dict(load_golden("g3_unet_d32c102")["shapes"], SEED)


def inputs():
    x = synth_input("window_once.x", (3, 4, H, W), SEED)
    return x, torch.tensor([3.5, 420.0, 997.0]), torch.tensor([64, 0, 101])


def build_model(sd, dev="cuda:0"):
    from flocoder_amd.unet import Unet
    m = Unet(dim=32, dim_mults=(1, 2, 4, 8), channels=4, n_classes=102).eval()
    m.load_state_dict(sd, strict=True)
    return m.to(dev)


def forward(m, x, t, cls, B, dev="cuda:0"):
    with torch.no_grad():
        return m(x[:B].to(dev), t[:B].to(dev), {"class_cond": cls[:B].to(dev)}).clone()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "window_once_parent.npz")
    sd = state_dict()
    x, t, cls = inputs()
    arrays, models = {}, {}
    for rows, B in CASES:
        if rows not in models:                 # (a reservation only grows: one model per plan size)
            models[rows] = build_model(sd)
            models[rows].reserve(rows, H, W)
        m = models[rows]
        assert m.reserved_rows() == rows
        arrays[f"v_rows{rows}_B{B}"] = forward(m, x, t, cls, B).cpu().numpy()
        assert m.fused_tail_errors() == 0
        assert any(r["kernel"].endswith("+fin") for r in m.profile_ops(B, repeats=1))
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
