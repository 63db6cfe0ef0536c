#!/usr/bin/env python3
"""tests/golden/codec_plan_parent.json: what the two codecs' plan builders emit, recorded ON THE BUILD BEFORE the builders were moved onto
PlanBuilder's shared verbs (csrc/plan.h: conv_on / layer / bind_out / finalize / activated), for tests/test_gpu_codec_plan_ledger.py to
compare exactly.  tests/golden/codec_pack_parent.npz pins what the codecs compute; a launch reordered or dropped without changing the bits
would pass there, so this pins the entries themselves, the way tests/golden/plan_ledger_parent.npz does for the U-Net.

    python tools/make_codec_plan_golden.py [out.json]        (needs the GPU; run it on a checkout of the commit to compare with)

The models and shapes are those of tools/make_codec_pack_golden.py (vae, vq, vq_na, each in fp32 and bf16x3; VAE 64x64, VQ 32x32, batch
2).  Per case, for the encode plan and the decode plan: every entry in order (kernel, module, FLOPs per sample, algorithmic bytes per
sample and per launch, as doubles -- JSON round-trips them exactly), the launch count and flops_per_sample.  Nothing runs: the plans are
reserved and their tables read.  The record belongs to one machine type, the MI355X: tile choice depends on the CU count.
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools import make_codec_pack_golden as pack   # noqa: E402

CASES = pack.CASES


def record(name):
    """Reserve both plans of a case -> {"encode": plan record, "decode": plan record}."""
    from flocoder_amd import _binding as B
    model, prec = name.split(".")
    m, zshape, hw = pack._model(model)
    m.set_precision(prec)
    hnd = m._native(torch.device(pack.DEV))
    out = {}
    for op, (h, w) in (("encode", (hw, hw)), ("decode", zshape[2:])):
        decode = op == "decode"
        B.check(m._fn("reserve_" + op)(hnd, 2, h, w))
        entries = [list(r) for r in m._plan_records(decode)]
        out[op] = {"entries": entries, "launches": int(m._fn("plan_launches")(hnd, int(decode))),
                   "flops_per_sample": m.flops_per_sample(decode)}
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "codec_plan_parent.json")
    meta = {}
    for name in CASES:
        meta[name] = record(name)
        for op, rec in meta[name].items():
            assert rec["launches"] == len(rec["entries"]) > 0 and rec["flops_per_sample"] > 0, (name, op)
        print(f"{name}: " + ", ".join(f"{op} {rec['launches']} launches, {rec['flops_per_sample'] / 1e9:.4f} GFLOP/sample" for op, rec in meta[name].items()))
    with open(out, "w") as f:
        json.dump(meta, f, separators=(",", ":"))
        f.write("\n")
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
