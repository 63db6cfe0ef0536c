"""Every tapped module of the U-Net forward, per sample, against an fp64 reference computed from the GPU's own input taps
(tests/unet_taps.py; the gates are documented there).  The whole-network rel-L2 of tests/test_gpu_unet.py dilutes a module's error by the
rest of the network and a sample's by its batch mates; here each (module, sample) answers for itself:

    module output   rel-L2 <= 2e-6 per sample
    residual branch ||out - ref|| <= 3e-6 ||ref - x|| + 2^-22 ||out||  per sample (linear / mid attention, ResnetBlocks with cin == cout)

(measured on one MI355X: worst module 5.1e-7, worst branch 6.1e-7).

The cases together put every forward kernel form of the planner on the path: each names the launches it exists for (read from the plan,
fc_unet_op_info) and asserts them, and the last test asserts that the union covers FORWARD_KERNELS.  The one-workgroup-per-sample kernel
(unet_sample.hip) has no taps: its output is gated per sample against the fp64 oracle.  With -s every case prints its worst errors."""
import ctypes as C
import re

import pytest
import torch

import unet_taps as ut
from conftest import load_golden, rel_l2
from oracle import flow_oracle as fo
from oracle.synth import synth_input, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_TOL = 2e-5

# launch names of the forward plans, templates stripped (conv_igemm<M128,N32> -> conv_igemm); "+fin": the launch closes its module
# (GroupNorm + FiLM + SiLU + residual, or GroupNorm(1) + residual) after its workgroups meet
FORWARD_KERNELS = {"temb", "ss", "init_conv", "mask_fusion(3 x conv_igemm)", "conv_igemm", "conv_igemm+fin", "bilinear+conv_igemm",
                   "finalize", "linattn_fused", "linattn_fused+fin", "linattn_sample", "linattn_ctx", "linattn_apply", "attn_sample",
                   "attn_small", "final_conv"}


def plan_kernels(model):
    from flocoder_amd import _binding as B
    out = set()
    for i in range(model.launches_per_forward):
        k = C.c_char_p()
        B.check(B.lib().fc_unet_op_info(model._handle, i, C.byref(k), None, None))
        out.add(re.sub(r"<[^>]*>", "", k.value.decode()))
    return out


def _sd(tag, seed, dim=None, n_classes=10):
    if tag is not None:
        return synth_state_dict(load_golden("g3_unet_" + tag)["shapes"], seed)
    from flocoder_amd.unet import Unet                                        # other widths: the same recipe over the model's own table
    shapes = {k: tuple(v.shape) for k, v in Unet(dim=dim, dim_mults=(1, 2, 4, 8), channels=4, n_classes=n_classes).state_dict().items()}
    return synth_state_dict(shapes, seed)


def _model(sd, mask_cond=False):
    from flocoder_amd.unet import Unet
    m = fo.unet_meta(sd)
    model = Unet(dim=m["dim"], dim_mults=(1, 2, 4, 8), channels=4, n_classes=m["n_classes"], mask_cond=mask_cond).eval()
    model.load_state_dict(sd, strict=True)
    return model.to(DEV)


# id: (shape table, seed, B, H, W, conditioning, plan, launches the case exists for)
CASES = {
    "d32c102-B1": ("d32c102", 1, 1, 32, 32, "class", "exclusive", {"linattn_fused+fin", "linattn_sample", "attn_sample", "conv_igemm+fin"}),
    "d32c102-B5": ("d32c102", 1, 5, 32, 32, "class", "exclusive", {"linattn_fused+fin", "linattn_sample", "attn_sample", "conv_igemm+fin"}),
    "d32c102-B17": ("d32c102", 1, 17, 32, 32, "class", "exclusive", {"linattn_fused+fin", "linattn_sample", "attn_sample", "conv_igemm+fin"}),
    "d32c102-B64-no-meeting": ("d32c102", 1, 64, 32, 32, "class", "fused_tail_off", {"linattn_fused", "finalize"}),
    "d32c102-B64-fin": ("d32c102", 1, 64, 32, 32, "class", "exclusive", {"linattn_fused+fin", "conv_igemm+fin"}),
    "d32c102-B5-shared": ("d32c102", 1, 5, 32, 32, "class", "shared", {"linattn_fused", "finalize"}),
    "d32c102-B3-train": ("d32c102", 1, 3, 32, 32, "class", "train", {"linattn_ctx", "linattn_apply", "attn_small", "finalize", "conv_igemm"}),
    "d32-64x64": ("d32c102", 4, 2, 64, 64, "class", "exclusive", {"linattn_fused+fin", "linattn_sample", "attn_sample"}),
    "d32-32x16": ("d32c102", 5, 3, 32, 16, "class", "exclusive", {"linattn_ctx", "linattn_apply", "linattn_sample"}),
    "d64-16x16": (None, 6, 2, 16, 16, "class", "exclusive", {"linattn_sample", "attn_sample"}),
    "d16c10-nocond": ("d16c10", 2, 3, 16, 16, None, "exclusive", {"linattn_fused+fin"}),
    "d8mask-ordinary": ("d8mask", 3, "cus+1", 8, 8, "mask", "exclusive", {"init_conv", "mask_fusion(3 x conv_igemm)", "bilinear+conv_igemm"}),
}
_SEEN = {}


def run_case(cid):
    from flocoder_amd import _binding as B
    from flocoder_amd._ops import fetch_tap
    tag, seed, bsz, H, W, cond_kind, plan, needs = CASES[cid]
    sd = _sd(tag, seed, dim=64)
    if bsz == "cus+1":                              # more samples than CUs: the ordinary plan, not the one-workgroup-per-sample kernel
        bsz = torch.cuda.get_device_properties(0).multi_processor_count + 1
    model = _model(sd, mask_cond="mask_fusion_conv.0.weight" in sd)
    g = torch.Generator().manual_seed(1000 + seed)
    x = synth_input(f"mp.{cid}", (bsz, 4, H, W), seed)
    t = torch.rand(bsz, generator=g) * 999
    t[0] = 0.999                                    # the sampler's first evaluation
    cond = None
    if cond_kind == "class":
        cond = {"class_cond": torch.randint(0, fo.unet_meta(sd)["n_classes"], (bsz,), generator=g)}
    elif cond_kind == "mask":
        cond = {"mask_cond": (torch.rand(bsz, 4, H, W, generator=g) > 0.35).float()}
    cd = None if cond is None else {k: v.to(DEV) for k, v in cond.items()}
    names = [m.name for m in ut.modules(sd, masked=cond_kind == "mask")][:-1]
    if plan == "train":
        names += [n for m in ut.modules(sd) if m.name in names for n in (m.name + s for s in m.internal)]
    stream = torch.cuda.Stream(DEV) if plan == "shared" else torch.cuda.current_stream(DEV)
    if plan == "fused_tail_off":
        B.check(B.lib().fc_debug_set_fused_tail(0))
    try:
        if plan == "shared":
            model.set_shared_device(True)
        stream.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(stream):
            if plan == "train":
                model.train()
                with torch.enable_grad():
                    out = model(x.to(DEV), t.to(DEV), cd).detach()
            else:
                with torch.no_grad():
                    out = model(x.to(DEV), t.to(DEV), cd)
            got = {n: fetch_tap(model, n, bsz).cpu() for n in names}
            got["x"], got["out"] = x, out.cpu()
            kernels = plan_kernels(model)
            meets = model.meeting_launches
            assert model.fused_tail_errors() == 0
    finally:
        if plan == "fused_tail_off":
            B.check(B.lib().fc_debug_set_fused_tail(-1))      # back to the default: later tests in this process build default plans
    _SEEN[cid] = kernels
    sd64 = {k: v.double() for k, v in sd.items()}
    mask = ut.mask_of(sd, cond)
    refs = ut.local_references(sd64, ut.conditioning(sd, t, cond), got, mask, internal=plan == "train")
    rows = ut.gate(sd64, got, refs, masked=mask is not None)
    return rows, kernels, meets, bsz


@pytest.mark.parametrize("cid", list(CASES))
def test_every_module_and_sample_matches_its_fp64_reference(cid):
    rows, kernels, meets, bsz = run_case(cid)
    plan, needs = CASES[cid][6], CASES[cid][7]
    print(f"\n[{cid}] B={bsz}: {len(rows)} (tap, sample) rows; {ut.report(rows)}")
    assert needs <= kernels, f"{cid}: the plan no longer runs {sorted(needs - kernels)}; it runs {sorted(kernels)}"
    if plan in ("shared", "fused_tail_off", "train"):
        assert meets == 0 and not any(k.endswith("+fin") and k.startswith("linattn") for k in kernels), sorted(kernels)
    elif "linattn_fused+fin" in needs:
        assert meets > 0
    taps = {r.tap for r in rows}
    assert len({r.sample for r in rows}) == bsz and "out" in taps and "mid_attn" in taps
    if plan == "train":
        assert {n for n in taps if n.endswith(ut.INTERNAL)} >= {"downs.0.0.h1", "downs.0.0.h2", "ups.3.2.qkv", "ups.3.2.lao", "ups.3.2.y"}
    assert all(r.ok for r in rows), f"{cid}: {ut.report(rows)}"


def test_the_cases_cover_every_forward_kernel():
    """A planner change that moves a module to another launch form must not silently drop that form from the module-parity gate."""
    for cid in CASES:
        if cid not in _SEEN:                        # (this test run on its own)
            run_case(cid)
    seen = set().union(*_SEEN.values())
    print(f"\nlaunch forms gated: {sorted(seen)}")
    assert FORWARD_KERNELS <= seen, f"no case runs {sorted(FORWARD_KERNELS - seen)}"
    assert seen <= FORWARD_KERNELS | {"gn_fold", "gn_stats"}, f"launch forms without a module-parity case: {sorted(seen - FORWARD_KERNELS)}"


@pytest.mark.parametrize("bsz", [1, 5])
def test_one_workgroup_per_sample_kernel_per_sample_vs_oracle(bsz):
    """csrc/unet_sample.hip runs the whole forward of a sample in one workgroup and keeps no taps: its output, sample by sample, against
    the fp64 oracle -- with a mask that is not all ones (the fusion convs and the injections) and with none."""
    sd = synth_state_dict(load_golden("g3_unet_d8mask")["shapes"], 3)
    model = _model(sd, mask_cond=True)
    sd64 = {k: v.double() for k, v in sd.items()}
    g = torch.Generator().manual_seed(70 + bsz)
    x, t = synth_input(f"mp.sample.{bsz}", (bsz, 4, 8, 8), 3), torch.rand(bsz, generator=g) * 999
    for cond in ({"mask_cond": (torch.rand(bsz, 4, 8, 8, generator=g) > 0.35).float()}, None):
        with torch.no_grad():
            out = model(x.to(DEV), t.to(DEV), None if cond is None else {"mask_cond": cond["mask_cond"].to(DEV)}).cpu()
        assert model.launches_per_forward <= 4, model.launches_per_forward              # conditioning + the ONE U-Net launch
        c64 = None if cond is None else {"mask_cond": cond["mask_cond"].double()}
        ref = fo.unet_forward(sd64, x.double(), t.double(), c64)
        errs = [rel_l2(out[b], ref[b]) for b in range(bsz)]
        print(f"\n[unet_sample B={bsz} {'mask' if cond else 'none'}] worst sample {max(errs):.2e} (sample {errs.index(max(errs))})")
        assert max(errs) < FWD_TOL, errs
