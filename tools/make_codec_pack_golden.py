#!/usr/bin/env python3
"""tests/golden/codec_pack_parent.npz: what the two native codecs compute from their packed weights, recorded ON THE BUILD BEFORE the
weight layouts were described once (csrc/common.h `PackKind`, one constructor per layout), for tests/test_gpu_codec_pack_ledger.py to
compare exactly.  The U-Net's wiring of the layouts is pinned by tests/golden/plan_ledger_parent.npz; this is the same for the codecs.

    python tools/make_codec_pack_golden.py [out.npz]        (needs the GPU; run it on a checkout of the commit to compare with)

Cases, each in "fp32" and in "bf16x3" (the latter reads the split-bf16 copies and the split folded-upsample kernels):

  vae     SD_VAE_Wrapper(weights="random", seed=7), RGB 64x64, batch 2: encode -> [2, 4, 8, 8], decode of a seeded latent -> [2, 3, 64, 64].
          The native AutoencoderKL has ONE configuration (block_out_channels (128, 256, 512, 512), two layers per block); a two-level
          (32, 64) model cannot be built on the parent, so the smallness is in the image: 64x64 is the smallest the parent takes (the
          mid-block attention's per-sample GEMMs refuse the 16 tokens of a 32x32 image).  Channel-padded conv_in / conv_out with the
          padded bias, plain and split-bf16 convolutions, the transposed Linears of the mid-block attention, the folded upsample in
          both forms.
  vq      VQVAE(in_channels=3, hidden_channels=32, num_downsamples=1, internal_dim=32, vq_embedding_dim=4, decoder_nonlocal=True), RGB
          32x32, batch 2: one downsample, a 'full' attention block at 16x16 in the decoder.  Channel-padded convolutions at both pixel
          ends and the 1x1 of the strided shortcut.
  vq_na   the same with natten_layout=1 and decoder_nonlocal=False, every NATTENBlock's gate opened to 0.8: the bias-free transposed
          Linears (qkv, proj).

Weights are what torch.manual_seed(0) draws (the VAE's come from its own seeded generator), inputs come from seeded CPU generators.  While
the tool runs (on the parent) every case runs twice; a tensor that did not reproduce bit for bit is left out and named under "unstable"
-- the fp64 gates of tests/test_gpu_codec_module_parity.py cover those.  The record belongs to one machine type, the MI355X: tile choice
depends on the CU count.
"""
import functools
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
VQ_CFG = dict(in_channels=3, hidden_channels=32, num_downsamples=1, internal_dim=32, vq_embedding_dim=4)


def _vae():
    from flocoder_amd.codecs import SD_VAE_Wrapper
    return SD_VAE_Wrapper(weights="random", seed=7).eval().to(DEV), (2, 4, 8, 8), 64


def _vq(natten):
    from flocoder_amd.codecs import VQVAE
    torch.manual_seed(0)
    m = VQVAE(natten_layout=1 if natten else 0, decoder_nonlocal=not natten, **VQ_CFG).eval()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith(".attn.gamma"):
                p.fill_(0.8)                        # the gate starts closed; open it so the attention's weights matter
    m.mark_dirty()
    return m.to(DEV), (2, 4, 16, 16), 32


MODELS = {"vae": _vae, "vq": lambda: _vq(False), "vq_na": lambda: _vq(True)}


@functools.lru_cache(maxsize=None)
def _model(name):
    """One model per process and name: both precisions read the same packed weights."""
    return MODELS[name]()


CASES =[f"{m}.{p}" for m in MODELS for p in ("fp32", "bf16x3")]


def record(name):
    """Run a case once -> {"encode": CPU tensor, "decode": CPU tensor}."""
    model, prec = name.split(".")
    m, zshape, hw = _model(model)
    m.set_precision(prec)
    g = torch.Generator().manual_seed(21 + CASES.index(name))
    x = torch.rand(2, 3, hw, hw, generator=g) * 2 - 1
    z = torch.randn(zshape, generator=g)
    out = {"encode": m.encode(x.to(DEV)).cpu(), "decode": m.decode(z.to(DEV)).cpu()}
    torch.cuda.synchronize()
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "codec_pack_parent.npz")
    arrays, meta = {}, {}
    for name in CASES:
        a, b = record(name), record(name)
        unstable = [k for k in a if not torch.equal(a[k], b[k])]
        meta[name] = {"unstable": unstable}
        for k, v in a.items():
            assert bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0, (name, k)
            if k not in unstable:
                arrays[f"{name}/{k}"] = v.numpy()
        print(f"{name}: " + ", ".join(f"{k} {tuple(v.shape)} |max| {float(v.abs().max()):.3g}" for k, v in a.items()) + f", unstable {unstable}")
    arrays["ledger"] = np.array(json.dumps(meta, separators=(",", ":")))
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
