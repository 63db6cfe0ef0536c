#!/usr/bin/env python3
"""tests/golden/conv_routes_parent.json: which conv_pipe_kernel instantiation every pipelined convolution launch goes to, recorded ON THE
BUILD BEFORE the instantiation table of conv_pipe.hip, for tests/test_gpu_conv_routes.py to compare exactly.

    python tools/make_conv_routes_golden.py [out.json]        (needs the GPU; run it on a checkout of the commit to compare with)

Routing is host logic -- a function of the launch's shapes, the plan's form and the runtime's occupancy answers, never of the data -- so
the record is pinned as it is.  Per case: the plan's entry kernel names (`+fin` shows what the occupancy query decided), the conv route
record (fc_debug_conv_routes: the thirteen template arguments per launch) and the step-route record.  A case stores its distinct
instantiations once and the launches as indices into them.  Weights are whatever seed 0 draws: no launch's route reads them.

The record belongs to one machine type, the MI355X with its 256 CUs: the occupancy answers and the tiles chosen for a grid depend on the
CU count, and the mask case's batch is that count plus one.  Record and compare on the same type.
"""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
ROWS = 64


def _unet(dim, H=32, W=32, rows=ROWS, shared=None, n_classes=102, train=False, **kw):
    from flocoder_amd.unet import Unet
    torch.manual_seed(0)
    m = Unet(dim=dim, dim_mults=(1, 2, 4, 8), channels=4, n_classes=n_classes, **kw)
    m = (m.train() if train else m.eval()).to(DEV)
    if shared is not None:
        m.set_shared_device(shared)
    if rows:
        m.reserve(rows, H, W)
    return m


def _inputs(B, H=32, W=32, n_classes=102):
    g = torch.Generator().manual_seed(B * 1000 + H)
    x = torch.randn(B, 4, H, W, generator=g).to(DEV)
    t = torch.linspace(1.0, 998.0, B).to(DEV)
    cls = ((torch.arange(B) * 37 + 5) % n_classes).to(DEV) if n_classes else None
    return x, t, cls


def _forward(m, B, H=32, W=32, n_classes=102, mask=None):
    x, t, cls = _inputs(B, H, W, n_classes)
    with torch.no_grad():
        m(x, t, {"class_cond": cls, "mask_cond": mask})
    return [r["kernel"] for r in m.profile_ops(B, repeats=1)]


def case_exclusive():
    """dim 32, plan of 64 rows at 4x32x32, B = 5, exclusive plan: every geometry flavour, whole-window forms."""
    return _forward(_unet(32, shared=False), 5)


def case_shared():
    """The same model on a shared device: no meeting flavours."""
    return _forward(_unet(32, shared=True), 5)


def case_euler():
    """The same model, two replayed Euler steps: the step-closing flavour and the step-route lines."""
    from flocoder_amd import sampling as S
    m = _unet(32, shared=False)
    x, _, cls = _inputs(3)
    S.euler_sampler(m, tuple(x.shape), 2, cond={"class_cond": cls}, source=x)
    return [r["kernel"] for r in m.profile_ops(3, repeats=1)]


def case_dim16():
    """dim 16, 64 rows at 4x32x32 and at 4x8x8, B = 3: run-time-geometry lean flavours, tiles of several samples."""
    m = _unet(16, n_classes=10)
    names = _forward(m, 3, n_classes=10)
    m.reserve(ROWS, 8, 8)
    return names + _forward(m, 3, 8, 8, n_classes=10)


def case_train():
    """One FlowTrainer.step at dim 32, B = 4, 4x16x16: the training plan and the data-gradient launches."""
    from flocoder_amd.train import FlowTrainer
    m = _unet(32, rows=0, train=True)
    g = torch.Generator().manual_seed(4)
    src, tgt = torch.randn(4, 4, 16, 16, generator=g), torch.randn(4, 4, 16, 16, generator=g)
    FlowTrainer(m, lr=1e-4).step(src, tgt, {"class_cond": torch.tensor([3, 77, 0, 101])}, u=torch.rand(4, generator=g))
    from flocoder_amd import _binding as Bd         # (the names alone: profile_ops times the plan on the sampler's buffers)
    lib, names = Bd.lib(), []
    for i in range(lib.fc_unet_plan_launches(m._handle)):
        k = C.c_char_p()
        Bd.check(lib.fc_unet_op_info(m._handle, i, C.byref(k), None, None))
        names.append(k.value.decode())
    return names


def case_mask():
    """A mask-conditioned forward (dim 8, 4x8x8) and a MaskEncoder forward (1x128x128): the remaining kernel sizes, cat / post flavours.
    One sample more than the device has CUs: the launch-per-layer plan, not the one-workgroup-per-sample kernel, which launches no
    convolution."""
    from flocoder_amd.inpainting import MaskEncoder
    m = _unet(8, rows=0, n_classes=0, mask_cond=True)
    g = torch.Generator().manual_seed(6)
    B = torch.cuda.get_device_properties(0).multi_processor_count + 1
    names = _forward(m, B, 8, 8, n_classes=0, mask=torch.rand(B, 4, 8, 8, generator=g).to(DEV))
    torch.manual_seed(0)
    with torch.no_grad():
        MaskEncoder().eval().to(DEV)((torch.rand(2, 1, 128, 128, generator=g) > 0.5).float().to(DEV))
    return names


def case_vqvae():
    """VQVAE encode + decode at 2x3x32x32: the all-in-one kernel at 1x1 and 3x3, on the 64-row and 32-row tiles these grids get.  (Two
    downsamplings: the decoder's attention needs the 8x8 latents -- a tile's 32 pixels per sample.  No case here fills the grids of
    the 64-column tiles: M256N64 and the lean 1x1 rows of M128N64 / M256N64 are not in the record.)"""
    from flocoder_amd.codecs import VQVAE
    torch.manual_seed(0)
    m = VQVAE(in_channels=3, hidden_channels=256, num_downsamples=2, internal_dim=128, vq_embedding_dim=4).eval().to(DEV)
    g = torch.Generator().manual_seed(7)
    z = m.encode(torch.rand(2, 3, 32, 32, generator=g).to(DEV))
    m.decode(torch.randn(tuple(z.shape), generator=g).to(DEV))
    return m.plan_kernels(decode=False) + m.plan_kernels(decode=True)


def case_sdvae():
    """SD-VAE encode + decode at 1x3x128x128, in fp32 and at set_precision("bf16x3"): the split-bf16 rows of M128N32, folded upsampling.
    (The smallest image whose layers fill the grid of a 128-row tile, the smallest with a split-bf16 form; below 64x64 the codec's
    attention refuses.)"""
    from flocoder_amd.codecs import SD_VAE_Wrapper
    w = SD_VAE_Wrapper(weights="random", seed=7).eval().to(DEV)
    g = torch.Generator().manual_seed(8)
    x = (torch.rand(1, 3, 128, 128, generator=g) * 2 - 1).to(DEV)
    names = []
    for prec in ("fp32", "bf16x3"):
        w.set_precision(prec)
        w.decode(w.encode(x))
        names += w.plan_kernels(decode=False) + w.plan_kernels(decode=True)
    return names


CASES = {"exclusive": case_exclusive, "shared": case_shared, "euler": case_euler, "dim16": case_dim16, "train": case_train,
         "mask": case_mask, "vqvae": case_vqvae, "sdvae": case_sdvae}


def record(name):
    """Run a case with the route records on -> {"kernels": plan entry names, "instantiations": distinct template-argument tuples,
    "launches": index of every conv launch's instantiation, in launch order, "steps": the step-route lines}."""
    from flocoder_amd import _binding as Bd
    lib = Bd.lib()
    Bd.check(lib.fc_debug_conv_routes(1))
    try:
        kernels = CASES[name]()
        torch.cuda.synchronize()
    finally:
        Bd.check(lib.fc_debug_conv_routes(0))
    texts = []
    for read in (lib.fc_debug_conv_routes_read, lib.fc_debug_step_routes_read):
        n = read(None, 0)
        buf = C.create_string_buffer(n + 1)
        read(buf, n + 1)
        texts.append(buf.value.decode().splitlines())
    launches = [[int(v) for v in line.split()] for line in texts[0]]
    distinct = sorted({tuple(r) for r in launches})
    index = {r: i for i, r in enumerate(distinct)}
    return {"kernels": kernels, "instantiations": [list(r) for r in distinct], "launches": [index[tuple(r)] for r in launches],
            "steps": texts[1]}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "conv_routes_parent.json")
    data = {name: record(name) for name in CASES}
    for name, rec in data.items():
        print(f"{name}: {len(rec['kernels'])} plan entries, {len(rec['launches'])} conv launches on {len(rec['instantiations'])} "
              f"instantiations, {len(rec['steps'])} step-route lines")
    with open(out, "w") as f:
        json.dump(data, f, separators=(",", ":"))
        f.write("\n")
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
