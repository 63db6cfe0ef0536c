#!/usr/bin/env python3
"""Per-launch table of the SD-VAE decoder (or encoder with --encode) at the sampler's shape: latents 4x32x32 -> 3x256x256."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flocoder_amd.codecs import SD_VAE_Wrapper

dev = torch.device("cuda", 0)
enc = "--encode" in sys.argv
bsz = int(os.environ.get("B", 16))
vae = SD_VAE_Wrapper(weights="random", seed=0).eval().to(dev)
z = torch.randn(bsz, 4, 32, 32, device=dev) * 4.5
img = vae.decode(z)
inp, out = (img, vae.encode(img)) if enc else (z, img)
rows = vae.profile_ops(inp, out, decode=not enc)
tot = sum(r["ms"] for r in rows)
print(f"{'module':46s} {'kernel':26s} {'ms':>8s} {'TFLOP/s':>8s}")
for r in rows:
    print(f"{r['module']:46s} {r['kernel']:26s} {r['ms']:8.3f} {r['flops_per_sample'] * bsz / max(r['ms'], 1e-9) / 1e9:8.1f}")
print("total ms", tot, "batch", bsz, "images/s", bsz / tot * 1e3)
