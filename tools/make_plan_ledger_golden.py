#!/usr/bin/env python3
"""tests/golden/plan_ledger_parent.npz: what the U-Net's plan builders emit and what the plans compute, recorded ON THE BUILD BEFORE the
builders walked the topology through csrc/unet_walk.h, for tests/test_gpu_plan_ledger.py to compare exactly.

    python tools/make_plan_ledger_golden.py [out.npz]        (needs the GPU; run it on a checkout of the commit to compare with)

Per case: the parameter table (names, shapes, offsets), every forward-plan entry (kernel, module, FLOPs and algorithmic bytes per sample /
per launch), flops_per_sample, launches_per_forward, meeting_launches and chains, for the training cases the backward plan's entries and
the subset fc_unet_vjp_x runs (what is missing from it carries the param-only flag), and the output tensors.  The cases are the smallest
that reach every branch of the walk: four levels with meeting launches and the step-closing head (A), the same on a shared device (B), a
training plan with its backward (C), the one-launch LDS program with a mask, an all-ones mask and no mask (D), the ordinary plan of the
same mask model (E), a non-square latent (F) and the two-level edge of the `i < 2 && i < L` injection condition in training form (G).

Weights are what torch.manual_seed(0) draws, inputs come from seeded CPU generators.  Forward outputs, d(x) and d(mask) are stored whole.
The flat parameter-gradient vector of case C has millions of elements, so gradients are stored as one SHA-256 digest per parameter (of its
fp32 bytes): equal digests are equal bits, and a mismatch names the parameter.  While the tool runs (on the parent) every gradient-
producing call runs twice; a tensor or a parameter's gradient that did not reproduce bit for bit is left out of the comparison and named
in the case's "unstable" list -- the fp64 gates of tests/test_gpu_unet_backward_parity.py cover those.

The record belongs to one machine type, the MI355X with its 256 CUs: the occupancy answers behind `+fin`, the tiles chosen for a grid,
which models get the one-launch plan and case E's reservation (the CU count plus one) depend on the CU count.  Record and compare on the
same type.
"""
import ctypes as C
import hashlib
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"


def _unet(dim, mults=(1, 2, 4, 8), n_classes=10, train=False, shared=None, **kw):
    from flocoder_amd.unet import Unet
    torch.manual_seed(0)
    m = Unet(dim=dim, dim_mults=mults, channels=4, n_classes=n_classes, **kw)
    m = (m.train() if train else m.eval()).to(DEV)
    if shared is not None:
        m.set_shared_device(shared)
    return m


def _inputs(seed, B, H, W, n_classes):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, H, W, generator=g)
    t = torch.rand(B, generator=g) * 999
    cls = torch.randint(0, n_classes, (B,), generator=g) if n_classes else None
    mask = (torch.rand(B, 4, H, W, generator=g) > 0.35).float()
    d_out = torch.randn(B, 4, H, W, generator=g)
    return x.to(DEV), t.to(DEV), None if cls is None else cls.to(DEV), mask.to(DEV), d_out.to(DEV)


def _names(count, info, handle):
    out = []
    for i in range(count(handle)):
        k, m = C.c_char_p(), C.c_char_p()
        info(handle, i, C.byref(k), C.byref(m))
        out.append([k.value.decode(), m.value.decode()])
    return out


def _ledger(m, backward=False):
    """The host-side record of the model's current plans."""
    from flocoder_amd import _binding as Bd
    lib, h = Bd.lib(), m._handle
    entries = []
    for i in range(lib.fc_unet_plan_launches(h)):
        k, mod, f, bp, bf = C.c_char_p(), C.c_char_p(), C.c_double(), C.c_double(), C.c_double()
        Bd.check(lib.fc_unet_op_info(h, i, C.byref(k), C.byref(mod), C.byref(f)))
        Bd.check(lib.fc_unet_op_bytes(h, i, C.byref(bp), C.byref(bf)))
        entries.append([k.value.decode(), mod.value.decode(), f.value, bp.value, bf.value])
    rec = {"params": [[n, list(s), int(o)] for n, s, o in m._table], "entries": entries, "flops_per_sample": m.flops_per_sample,
           "launches_per_forward": m.launches_per_forward, "meeting_launches": m.meeting_launches, "chains": list(m.chains)}
    if backward:
        rec["backward"] = _names(lib.fc_unet_backward_launches, lib.fc_unet_backward_op_info, h)
        rec["vjp"] = _names(lib.fc_unet_vjp_launches, lib.fc_unet_vjp_op_info, h)
    return rec


def _digests(m, flat):
    host = flat.detach().cpu().numpy()
    return {n: hashlib.sha256(host[o:o + math.prod(s)].tobytes()).hexdigest() for n, s, o in m._table}


def _inference(m, rows, B, H, W, seed, masks=(None,)):
    n_classes = int(m._cfg.n_classes)
    x, t, cls, mask, _ = _inputs(seed, B, H, W, n_classes)
    m.reserve(rows, H, W)
    tensors = {}
    with torch.no_grad():
        for kind in masks:
            mk = {None: None, "mask": mask, "ones": torch.ones_like(mask)}[kind]
            tensors["out" if kind is None else "out." + kind] = m(x, t, {"class_cond": cls, "mask_cond": mk}).cpu()
    return _ledger(m), tensors


def _training(m, B, H, W, seed, masked):
    """Training-form forward, d(x) alone (fc_unet_vjp_x) and the full backward; each gradient-producing call twice."""
    n_classes = int(m._cfg.n_classes)
    x, t, cls, mask, d_out = _inputs(seed, B, H, W, n_classes)
    mk = mask if masked else None
    tensors = {"out": m._forward_native(x, t, cls, mk, train=True).cpu()}
    runs = []
    for _ in range(2):
        vjp = m.vjp_x(x, t, cls, d_out, mask=mk)
        flat, dx, dm = m.backward_native(x, t, cls, d_out, mask=mk, want_dx=True, want_dmask=masked)
        torch.cuda.synchronize()
        got = {"vjp_x": vjp.cpu(), "dx": dx.cpu()}
        if dm is not None:
            got["dmask"] = dm.cpu()
        runs.append((got, _digests(m, flat)))
    rec = _ledger(m, backward=True)
    unstable = [k for k in runs[0][0] if not torch.equal(runs[0][0][k], runs[1][0][k])]
    unstable += ["grad:" + n for n in runs[0][1] if runs[0][1][n] != runs[1][1][n]]
    tensors.update({k: v for k, v in runs[0][0].items() if k not in unstable})
    rec["grads"] = {n: d for n, d in runs[0][1].items() if "grad:" + n not in unstable}
    rec["unstable"] = unstable
    return rec, tensors


def case_a():
    """dim 32, four levels, 102 classes, 64 rows at 32x32, B = 5, exclusive device: meeting launches and the step-closing head."""
    return _inference(_unet(32, n_classes=102, shared=False), 64, 5, 32, 32, 11)


def case_b():
    """The same model on a shared device."""
    return _inference(_unet(32, n_classes=102, shared=True), 64, 5, 32, 32, 11)


def case_c():
    """dim 16, 10 classes, training form at 16x16, rows = B = 4: forward, vjp_x and a backward into a flat gradient vector."""
    return _training(_unet(16, n_classes=10, train=True), 4, 16, 16, 13, masked=False)


def case_d():
    """dim 8 with mask conditioning at 8x8, rows = B = 3: the one-launch plan with a mask, an all-ones mask and no mask."""
    return _inference(_unet(8, mask_cond=True), 3, 3, 8, 8, 14, masks=("mask", "ones", None))


def case_e():
    """The same model reserved for one row more than the device has CUs: the ordinary plan with both injections and the fusion."""
    rows = torch.cuda.get_device_properties(0).multi_processor_count + 1
    return _inference(_unet(8, mask_cond=True), rows, 3, 8, 8, 14, masks=("mask",))


def case_f():
    """dim 8 with mask conditioning on a non-square 4x8 latent: the one-launch plan.  Three levels, mults (1, 2, 4): as deep as four rows
    allow (the bottleneck runs at 1x2)."""
    return _inference(_unet(8, mults=(1, 2, 4), mask_cond=True), 3, 3, 4, 8, 16, masks=("mask",))


def case_g():
    """dim 8, mults (1, 2), mask conditioning, no classes, training form at 8x8, rows = B = 2: the L = 2 edge of `i < 2 && i < L`, the
    injection and fusion records on the tape for the backward."""
    return _training(_unet(8, mults=(1, 2), n_classes=0, train=True, mask_cond=True), 2, 8, 8, 17, masked=True)


CASES = {"A": case_a, "B": case_b, "C": case_c, "D": case_d, "E": case_e, "F": case_f, "G": case_g}


def record(name):
    """Run a case -> (ledger: a JSON-able dict, tensors: {name: CPU tensor})."""
    rec, tensors = CASES[name]()
    torch.cuda.synchronize()
    return rec, tensors


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "plan_ledger_parent.npz")
    arrays, meta = {}, {}
    for name in CASES:
        rec, tensors = record(name)
        meta[name] = rec
        for k, v in tensors.items():
            arrays[f"{name}/{k}"] = v.numpy()
        print(f"{name}: {len(rec['entries'])} forward entries ({rec['meeting_launches']} meet), {len(rec.get('backward', []))} backward, "
              f"{len(rec.get('vjp', []))} vjp, tensors {sorted(tensors)}, unstable {rec.get('unstable', [])}")
    arrays["ledger"] = np.array(json.dumps(meta, separators=(",", ":")))
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
