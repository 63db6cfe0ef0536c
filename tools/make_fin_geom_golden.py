#!/usr/bin/env python3
"""tests/golden/fin_geom_parent_fused.npz: forwards of the dim-32 U-Net with fused Block tails, recorded ON THE BUILD BEFORE the geometry
flavours of the Block-closing convolutions (conv_dev.h GEO), for tests/test_gpu_conv_fin_geom.py to compare bit for bit.

    python tools/make_fin_geom_golden.py [out.npz]            (needs the GPU; run it on a checkout of the commit to compare with)

The two-launch form (convolution + `finalize`) is NOT bit-equal to the fused tail -- `finalize` sums the GroupNorm(1) partials of the final
value in another order -- so the fused output of the earlier build is the reference.  Weights and inputs are the synthetic ones of the other
goldens (oracle/synth.py: a function of name, shape and seed only); plans are built for 64 rows, as bench.py's.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.synth import synth_input, synth_state_dict  # noqa: E402

ROWS, SEED = 64, 17
SIZES = [(8, 8), (16, 16), (32, 32)]
BATCHES = (3, 5)


def state_dict():
    from conftest import load_golden
    return synth_state_dict(load_golden("g3_unet_d32c102")["shapes"], SEED)


def inputs(H, W):
    x = synth_input(f"fin_geom.x.{H}x{W}", (5, 4, H, W), SEED)
    t = torch.tensor([0.999, 250.0, 500.5, 751.0, 998.0])
    return x, t, torch.tensor([101, 0, 37, 5, 77])


def build_model(sd, dev="cuda:0"):
    from flocoder_amd.unet import Unet
    m = Unet(dim=32, dim_mults=(1, 2, 4, 8), channels=4, n_classes=102).eval()
    m.load_state_dict(sd, strict=True)
    return m.to(dev)


def forward(m, x, t, cls, B, dev="cuda:0"):
    with torch.no_grad():
        return m(x[:B].to(dev), t[:B].to(dev), {"class_cond": cls[:B].to(dev)}).clone()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "fin_geom_parent_fused.npz")
    m = build_model(state_dict())
    arrays = {}
    for H, W in SIZES:
        x, t, cls = inputs(H, W)
        m.reserve(ROWS, H, W)
        for B in BATCHES:
            arrays[f"v_{H}x{W}_B{B}"] = forward(m, x, t, cls, B).cpu().numpy()
        assert m.fused_tail_errors() == 0
        assert any(r["kernel"].endswith("+fin") for r in m.profile_ops(5, repeats=1))
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
