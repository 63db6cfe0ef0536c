"""The fused linear attention's fast path (csrc/linattn_fused.hip: la_ctx_fast / la_apply_fast), whose MFMA phases hand their
accumulators on in registers with a permuted reduction order: every linear-attention tap of a U-Net forward, per sample, against the
fp64 local reference of tests/unet_taps.py, under the gates documented there (MODULE_TOL, BRANCH_TOL, STORE_FLOOR -- unchanged).

The shapes are the smallest that reach each instantiation and edge of the two kernels:

    dim 32, 32x32, B=3   C=32 at n=1024 and n=256 (la_ctx_fast<4,8>, la_apply_fast<4,1>), C=64 at n=256 (<8,8>, <8,2>: two output tiles)
    dim 16, 32x32, B=2   C=16 (<2,8>, <2,1>) and C=32 at n=256
    dim 32, 16x8,  B=3   n=128 at the first level.  The planner hands the fused kernels only n >= 256 (csrc/unet.hip), so this level runs
                         the unfused linattn_ctx / linattn_apply chain and the four-wave la_ctx_fast<.,4> is not reachable from a forward;
                         the case keeps the taps of that shape under the same gate

each on the exclusive plan (where the grid is resident the apply launch closes the module itself, "linattn_fused+fin") and on the shared
plan (no meeting: y and its statistics go through finalize).  Odd batch sizes, so that a sample-index or tile-index slip cannot cancel.
With -s every case prints its worst errors."""
import ctypes as C
import re

import pytest
import torch

import unet_taps as ut
from conftest import load_golden
from oracle import flow_oracle as fo
from oracle.synth import synth_input, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# id: (shape table, seed, B, H, W, attention taps that must run on linattn_fused)
SHAPES = {
    "d32-32x32-B3": ("d32c102", 11, 3, 32, 32, {"downs.0.2", "downs.1.2", "ups.2.2", "ups.3.2"}),
    "d16-32x32-B2": ("d16c10", 12, 2, 32, 32, {"downs.0.2", "downs.1.2", "ups.2.2", "ups.3.2"}),
    "d32-16x8-B3": ("d32c102", 13, 3, 16, 8, set()),
}


def _plan(model):
    """(launch name without templates, module) of every launch of the forward plan"""
    from flocoder_amd import _binding as B
    out = []
    for i in range(model.launches_per_forward):
        k = C.c_char_p()
        B.check(B.lib().fc_unet_op_info(model._handle, i, C.byref(k), None, None))
        out.append(re.sub(r"<[^>]*>", "", k.value.decode()))
    return out


def _model(tag, seed):
    from flocoder_amd.unet import Unet
    sd = synth_state_dict(load_golden("g3_unet_" + tag)["shapes"], seed)
    m = fo.unet_meta(sd)
    model = Unet(dim=m["dim"], dim_mults=(1, 2, 4, 8), channels=4, n_classes=m["n_classes"]).eval()
    model.load_state_dict(sd, strict=True)
    return sd, model.to(DEV)


def _forward_taps(sd, model, x, t, cls, shared):
    """One forward; every module's output tap (and the network's input and output) on the CPU."""
    from flocoder_amd._ops import fetch_tap
    bsz = x.shape[0]
    names = [m.name for m in ut.modules(sd)][:-1]
    stream = torch.cuda.Stream(DEV) if shared else torch.cuda.current_stream(DEV)
    if shared:
        model.set_shared_device(True)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream), torch.no_grad():
        out = model(x.to(DEV), t.to(DEV), {"class_cond": cls.to(DEV)})
        got = {n: fetch_tap(model, n, bsz).cpu() for n in names}
        got["x"], got["out"] = x, out.cpu()
        kernels, meets = _plan(model), model.meeting_launches
        assert model.fused_tail_errors() == 0
    return got, kernels, meets


@pytest.mark.parametrize("plan", ["exclusive", "shared"])
@pytest.mark.parametrize("cid", list(SHAPES))
def test_linear_attention_taps_match_their_fp64_reference(cid, plan):
    tag, seed, bsz, H, W, fused = SHAPES[cid]
    sd, model = _model(tag, seed)
    g = torch.Generator().manual_seed(2000 + seed)
    x = synth_input(f"lachain.{cid}", (bsz, 4, H, W), seed)
    t = torch.rand(bsz, generator=g) * 999
    cls = torch.randint(0, fo.unet_meta(sd)["n_classes"], (bsz,), generator=g)
    got, kernels, meets = _forward_taps(sd, model, x, t, cls, plan == "shared")
    n_fused = sum(k in ("linattn_fused", "linattn_fused+fin") for k in kernels)
    assert n_fused == len(fused), f"{cid}: {n_fused} fused linear-attention launches, expected {len(fused)}: {kernels}"
    if plan == "shared":
        assert meets == 0 and "linattn_fused+fin" not in kernels, kernels
    elif H * W >= 1024:
        assert "linattn_fused+fin" in kernels and meets > 0, kernels      # n >= 256 levels: the apply launch closes the module
    else:
        assert "linattn_ctx" in kernels and "linattn_apply" in kernels, kernels      # n = 128: the unfused chain
    sd64 = {k: v.double() for k, v in sd.items()}
    refs = ut.local_references(sd64, ut.conditioning(sd, t, {"class_cond": cls}), got)
    rows = [r for r in ut.gate(sd64, got, refs) if r.tap.endswith(".2")]
    print(f"\n[{cid} {plan}] {len(rows)} (attention tap, sample) rows; {ut.report(rows)}")
    assert {r.tap for r in rows} >= fused | {"downs.0.2", "ups.3.2"} and len({r.sample for r in rows}) == bsz
    assert all(r.branch == r.branch for r in rows)                         # every one of them has the branch gate too
    assert all(r.ok for r in rows), f"{cid} {plan}: {ut.report(rows)}"


def test_attention_output_does_not_depend_on_the_batch_or_the_position_in_it():
    """The same sample alone (B=1) and at positions 1 and 4 of a B=5 batch: wherever a fused attention module was handed bit-equal input
    and bit-equal statistics, its output is bit-equal.  Inside the batch that is every module; against B=1 at least the first one."""
    tag, seed = "d32c102", 14
    sd, model = _model(tag, seed)
    g = torch.Generator().manual_seed(2000 + seed)
    x5 = synth_input("lachain.batch", (5, 4, 32, 32), seed)
    t5 = torch.rand(5, generator=g) * 999
    c5 = torch.randint(0, fo.unet_meta(sd)["n_classes"], (5,), generator=g)
    x5[4], t5[4], c5[4] = x5[1], t5[1], c5[1]
    got5, kernels, _ = _forward_taps(sd, model, x5, t5, c5, False)
    assert "linattn_fused+fin" in kernels, kernels
    got1, _, _ = _forward_taps(sd, model, x5[1:2].clone(), t5[1:2].clone(), c5[1:2].clone(), False)
    taps = ["downs.0.2", "downs.1.2", "ups.2.2", "ups.3.2"]
    src = {m.name: m.inputs[0] for m in ut.modules(sd)}
    for n in taps:
        assert torch.equal(got5[src[n]][1], got5[src[n]][4]), f"{src[n]}: the input of {n} differs between positions 1 and 4"
        assert torch.equal(got5[n][1], got5[n][4]), f"{n}: positions 1 and 4 of one batch differ"
    same_in = [n for n in taps if torch.equal(got1[src[n]][0], got5[src[n]][1])]
    print(f"\nB=1 against B=5: bit-equal inputs at {same_in}")
    assert "downs.0.2" in same_in, "the first attention module's input differs between B=1 and B=5"
    for n in same_in:
        assert torch.equal(got1[n][0], got5[n][1]), f"{n}: B=1 and position 1 of B=5 differ on bit-equal input"
