"""Every activation gradient of the U-Net backward per (tap, sample), d(x) and d(mask) per sample, and every parameter gradient per tensor,
against fp64 module-local VJPs built from the GPU's own forward taps and output cotangents (tests/unet_grad_taps.py; the gates and
their tolerances are documented there).  tests/test_gpu_train.py compares each whole parameter gradient with fp32 autograd through the
whole network, where a sample's or a module's error is diluted by everything else; here each (tap, sample) answers for itself.

Every case first gates the forward taps (unet_taps.gate, internal taps included), so that the backward references rest on checked
inputs, then asserts the backward launch forms it exists for (read from the plan, fc_unet_backward_op_info); the last test asserts that
the cases together cover BACKWARD_KERNELS.  The output cotangent differs in scale by 1e2..1e-2 between samples (one case uses the MSE
gradient of the training step instead).  With -s every case prints its worst rows.

TRAIN_CASES gate the plans of the shipped training batches (256 and 2048 rows) the same way on 8 rows: the cotangent is zero on every
other row, whose gradients must then be zero to the bit, and the 8 rows' taps are gathered on the device.  Measured on the MI355X
(forward module / branch; backward activation / branch / parameter, parameter in rounding units):
    d32c102-B256   1.28e-6 / 1.26e-6;  6.11e-7 / 1.07e-7 / 2.16e-6, 19.6 u
    d16c10-B256    6.20e-7 / 6.04e-7;  3.43e-7 / 1.44e-7 / 1.21e-6, 11.7 u
    d8mask-B2048   5.32e-7 / 3.87e-7;  5.25e-7 / 1.02e-7 / 1.74e-6, 11.4 u
d32c102-B256 first measured a branch error of 4.92e-7 against the BRANCH_TOL of 4e-7 (grad:downs.3.3 rows 254 and 255, grad:mid_attn rows
8 and 254: the data gradients of mid_block1 / mid_block2's block1.proj, 256 -> 256 3x3 at 4x4).  At 256 rows auto_tile gave those launches
M128N32, one accumulation chain over K = 2304, where the small cases run M32N32K4, four chains of 576; the same convolution on dense
random data measures 7.4e-7 / 5.3e-7 / 2.7e-7 against fp64 on M128N32 / M64N32K2 / M32N32K4.  The backward's data gradients with 2048 or
more terms at <= 16 pixels per sample now take the four-chain tile at every batch (ConvArgs::split_long_k; also the faster tile there),
and the case passes at the figures above."""
import ctypes as C
import re

import pytest
import torch

import unet_grad_taps as gt
import unet_taps as ut
from conftest import load_golden
from oracle import flow_oracle as fo
from oracle.synth import synth_input, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# launch names of the backward plans (unet_backward.hip push(...) names, templates stripped); the attention core backward of the linear
# attention is split by its two forms (linattn_bwd_ctx_kernel<8,64> for n > 256 positions, <4,32> below)
BACKWARD_KERNELS = {"nchw_to_nhwc", "nhwc_to_nchw", "memset", "conv_igemm", "conv_wgrad", "conv_wgrad_table", "wgrad_reduce", "finalize",
                    "finalize_table", "gn_bwd", "norm_param_grads", "add_into", "copy", "linattn_bwd(n>256)", "linattn_bwd(n<=256)",
                    "attn_small_bwd", "depth_to_space", "sumpool2", "silu_bwd", "bilinear_bwd", "dgrad(init_conv)", "dense_bwd_w",
                    "dense_bwd_x", "time_mlp_bwd", "class_mlp_bwd"}


def _level_hw(module, H, W, L):
    """Resolution a module's attention runs at."""
    if module == "mid_attn":
        return (H >> (L - 1)) * (W >> (L - 1))
    i = int(module.split(".")[1])
    lvl = i if module.startswith("downs.") else L - 1 - i
    return (H >> lvl) * (W >> lvl)


def backward_forms(model, H, W, L):
    """{(launch form, module)} of the model's backward plan."""
    from flocoder_amd import _binding as B
    lib = B.lib()
    out = set()
    for i in range(lib.fc_unet_backward_launches(model._handle)):
        k, m = C.c_char_p(), C.c_char_p()
        B.check(lib.fc_unet_backward_op_info(model._handle, i, C.byref(k), C.byref(m)))
        k, m = re.sub(r"<[^>]*>", "", k.value.decode()), m.value.decode()
        if k == "linattn_bwd":
            k += "(n>256)" if _level_hw(m, H, W, L) > 256 else "(n<=256)"
        out.add((k, m))
    return out


def _model(sd, mask_cond=False):
    from flocoder_amd.unet import Unet
    m = fo.unet_meta(sd)
    model = Unet(dim=m["dim"], dim_mults=(1, 2, 4, 8), channels=4, n_classes=m["n_classes"], mask_cond=mask_cond)
    model.load_state_dict(sd, strict=True)
    return model.to(DEV).train()


# id: (shape table, seed, B, H, W, conditioning, variant, launch forms the case exists for (kernel, or (kernel, module)))
#   variant: "" | "mse" (d_out = the MSE gradient) | "short" (reserved at B=8, stepped at B) | "buckets" (two-bucket plan, parts
#   (0,0)+(1,1)) | "mask", "mask-ones", "mask-none" (the mask plan with a mask not all ones / all ones / no mask)
CASES = {
    "d32c102-B3": ("d32c102", 1, 3, 32, 32, "class", "", {("linattn_bwd(n>256)", "downs.0.2"), ("linattn_bwd(n<=256)", "downs.2.2"),
                                                           ("attn_small_bwd", "mid_attn"), "depth_to_space", "sumpool2", "class_mlp_bwd",
                                                           "conv_wgrad_table", "wgrad_reduce", "finalize_table"}),
    "d16c10-B8-mse": ("d16c10", 2, 8, 16, 16, "class", "mse", {"linattn_bwd(n<=256)", "attn_small_bwd", "class_mlp_bwd"}),
    "d16c10-B8-nocond": ("d16c10", 2, 8, 16, 16, None, "", {"time_mlp_bwd", "class_mlp_bwd"}),
    "d16c10-B5-of-8": ("d16c10", 2, 5, 16, 16, "class", "short", {"conv_wgrad", "finalize"}),
    "d32-64x64": ("d32c102", 4, 2, 64, 64, "class", "", {("attn_small_bwd", "mid_attn"), ("linattn_bwd(n>256)", "ups.3.2")}),
    "d32-32x16": ("d32c102", 5, 3, 32, 16, "class", "", {"linattn_bwd(n>256)", "linattn_bwd(n<=256)"}),
    "d8mask": ("d8mask", 3, 3, 8, 8, "mask", "mask", {"silu_bwd", "bilinear_bwd", "nhwc_to_nchw", "memset", "copy", "add_into"}),
    "d8mask-ones": ("d8mask", 3, 3, 8, 8, "mask", "mask-ones", {"bilinear_bwd"}),
    "d8mask-none": ("d8mask", 3, 3, 8, 8, "mask", "mask-none", {"silu_bwd"}),
    "d32c102-B3-buckets": ("d32c102", 1, 3, 32, 32, "class", "buckets", {"conv_wgrad_table", "norm_param_grads", "dense_bwd_w"}),
}
_SEEN = {}


def run_case(cid):
    from flocoder_amd._ops import fetch_tap
    from flocoder_amd import _binding as B
    tag, seed, bsz, H, W, cond_kind, variant, _ = CASES[cid]
    sd = synth_state_dict(load_golden("g3_unet_" + tag)["shapes"], seed)
    meta = fo.unet_meta(sd)
    masked = variant.startswith("mask")
    model = _model(sd, mask_cond=masked)
    if variant == "buckets":
        model.set_grad_buckets(True)
    g = torch.Generator().manual_seed(2000 + seed)
    x = synth_input(f"bp.{cid}", (bsz, 4, H, W), seed)
    t = torch.rand(bsz, generator=g) * 999
    cls = torch.randint(0, meta["n_classes"], (bsz,), generator=g) if cond_kind == "class" else None
    mask = None
    if variant == "mask":
        mask = (torch.rand(bsz, 4, H, W, generator=g) > 0.35).float()
    elif variant == "mask-ones":
        mask = torch.ones(bsz, 4, H, W)
    xd, td = x.to(DEV), t.to(DEV)
    cd = None if cls is None else cls.to(DEV)
    md = None if mask is None else mask.to(DEV)
    if variant == "short":                           # the plan is reserved for 8 rows; this step runs fewer
        model._forward_native(torch.zeros(8, 4, H, W, device=DEV), torch.zeros(8, device=DEV), None, None, train=True)
    out = model._forward_native(xd, td, cd, md, train=True)
    if variant == "mse":                             # d(mean((v - v*)^2)) / dv, the training step's own cotangent
        target = synth_input(f"bp.v.{cid}", (bsz, 4, H, W), seed).to(DEV)
        d_out = (2.0 / out.numel()) * (out - target)
    else:
        d_out = (synth_input(f"bp.d.{cid}", (bsz, 4, H, W), seed) * torch.logspace(2, -2, bsz).view(bsz, 1, 1, 1)).to(DEV)
    if variant == "buckets":
        assert model.grad_buckets()[0] == 2
        flat, dx, dm = model.backward_native(xd, td, cd, d_out, mask=md, want_dx=True, want_dmask=True, parts=(0, 0))
        model.backward_native(xd, td, cd, d_out, grads=flat, mask=md, want_dx=True, want_dmask=True, parts=(1, 1), dx=dx, dm=dm)
    else:
        flat, dx, dm = model.backward_native(xd, td, cd, d_out, mask=md, want_dx=True, want_dmask=True)
    torch.cuda.synchronize()
    rb, rh, rw = C.c_int(), C.c_int(), C.c_int()
    B.check(B.lib().fc_unet_reserved(model._handle, C.byref(rb), C.byref(rh), C.byref(rw)))
    mods = ut.modules(sd, masked=mask is not None)
    names = [m.name for m in mods][:-1]
    internal = [n for m in ut.modules(sd) if m.name in names for n in (m.name + s for s in m.internal)]
    got = {n: fetch_tap(model, n, bsz).cpu() for n in names + internal}
    got.update({"grad:" + n: fetch_tap(model, "grad:" + n, bsz).cpu() for n in names})
    got["x"], got["out"], got["dx"] = x, out.cpu(), dx.cpu()
    if dm is not None:
        got["dmask"] = dm.cpu()
    pgrads = {k: v.cpu() for k, v in model.grad_views(flat).items()}
    forms = backward_forms(model, H, W, meta["n_levels"])
    _SEEN[cid] = {k for k, _ in forms}

    sd64 = {k: v.double() for k, v in sd.items()}
    cond = {} if cls is None else {"class_cond": cls}
    if mask is not None:
        cond["mask_cond"] = mask
    temb = ut.conditioning(sd, t, cond or None)
    m64 = ut.mask_of(sd, cond)
    frows = ut.gate(sd64, got, ut.local_references(sd64, temb, got, m64, internal=True), masked=m64 is not None)
    refs = gt.local_vjp(sd64, temb, got, gt.cotangents(sd64, got, d_out.cpu(), masked=m64 is not None), t.double(), cls, m64)
    grows, prows = gt.gate_activations(got, refs), gt.gate_params(pgrads, refs)
    return dict(frows=frows, grows=grows, prows=prows, forms=forms, reserved=rb.value, refs=refs, pgrads=pgrads)


def _heavy(cid):
    return pytest.param(cid, marks=pytest.mark.timeout(120))     # ~0.5 s measured per case


@pytest.mark.parametrize("cid", [_heavy(c) for c in CASES])
def test_every_gradient_tap_sample_and_parameter_matches_its_fp64_local_vjp(cid):
    r = run_case(cid)
    bsz, variant, needs = CASES[cid][2], CASES[cid][6], CASES[cid][7]
    print(f"\n[{cid}] B={bsz}: forward {ut.report(r['frows'])}\n  backward {len(r['grows'])} (tap, sample) rows, {len(r['prows'])} "
          f"parameters; {gt.report(r['grows'], r['prows'])}")
    fin = [p for p in r["prows"] if p.scale > 0]
    print("  largest parameter errors: " + ", ".join(f"{p.name} {p.rel:.1e} ({p.scale:.1f} u)" for p in sorted(fin, key=lambda p: -p.rel)[:3])
          + "; in rounding units: " + ", ".join(f"{p.name} {p.scale:.1f} u ({p.rel:.1e})" for p in sorted(fin, key=lambda p: -p.scale)[:3]))
    assert all(row.ok for row in r["frows"]), f"{cid}: forward taps: {ut.report(r['frows'])}"
    kernels = {k for k, _ in r["forms"]}
    for n in needs:
        present = (n in r["forms"]) if isinstance(n, tuple) else (n in kernels)
        assert present, f"{cid}: the backward plan no longer runs {n}; it runs {sorted(kernels)}"
    taps = {row.tap for row in r["grows"]}
    assert {"dx", "grad:init", "grad:mid_attn", "grad:final_res_block"} <= taps and len({row.sample for row in r["grows"]}) == bsz
    if variant == "mask":
        assert "dmask" in taps and r["refs"].params["mask_fusion_conv.0.weight"] is not None
    if variant == "short":
        assert r["reserved"] == 8, r["reserved"]         # the plan stayed at 8 rows: this step ran the inline (non-table) forms
    if CASES[cid][5] is None:                            # no class conditioning: the class MLP's gradients are exactly zero
        cl = [k for k in r["pgrads"] if k.startswith("class_cond_mlp.")]
        assert cl and all(r["refs"].params[k] is None and not r["pgrads"][k].any() for k in cl)
    assert all(row.ok for row in r["grows"]) and all(row.ok for row in r["prows"]), f"{cid}: {gt.report(r['grows'], r['prows'])}"


# The shipped training batches (configs/common/flow.yaml and midi_vqgan.yaml: 256; midi_inpainting.yaml: 2048).  The plan is a function of
# the batch: auto_tile's block-count thresholds pick other tiles and with them other conv_pipe flavours, the low-resolution levels run
# multi-sample tiles (2, 8, 32 or 128 samples), and a weight-gradient workgroup walks several pixel tiles.  id: (shape table, seed, B, H, W,
# conditioning, variant)
TRAIN_CASES = {
    "d32c102-B256": ("d32c102", 1, 256, 32, 32, "class", ""),
    "d16c10-B256": ("d16c10", 2, 256, 16, 16, "class", ""),
    "d8mask-B2048": ("d8mask", 3, 2048, 8, 8, "mask", "mask"),
}


def plan_launch_names(model):
    """Template-qualified launch names of the model's forward plan and of its backward plan, in plan order."""
    from flocoder_amd import _binding as B
    lib = B.lib()
    fwd, bwd = [], []
    for i in range(lib.fc_unet_plan_launches(model._handle)):
        k, m, fl = C.c_char_p(), C.c_char_p(), C.c_double()
        B.check(lib.fc_unet_op_info(model._handle, i, C.byref(k), C.byref(m), C.byref(fl)))
        fwd.append(k.value.decode())
    for i in range(lib.fc_unet_backward_launches(model._handle)):
        k, m = C.c_char_p(), C.c_char_p()
        B.check(lib.fc_unet_backward_op_info(model._handle, i, C.byref(k), C.byref(m)))
        bwd.append(k.value.decode())
    return fwd, bwd


def subset_rows(bsz, H, W):
    """The rows that carry a cotangent, and what the launches' own geometry says about them: row 0 and row B-1; rows 0 and 1, which share a
    multi-sample weight-gradient tile at the deepest level, and rows B-2 and B-1, which share the last; rows TB-1 and TB, adjacent and in
    different tiles; and rows that fall into different weight-gradient splits at level 0.  The geometry is read from a stand-in launch of
    the 3x3 weight gradient at either level's resolution with the table entries' split target (4 channels: TB does not depend on the
    channel count, and level 0's own layers are one 32 x 32 block wide as well, so their split count is the stand-in's)."""
    from flocoder_amd._ops import conv_wgrad_debug

    def geo(h, w):
        z = torch.zeros(bsz, 4, h, w, device=DEV)
        return conv_wgrad_debug(z, z, 3, pad=1, split_target=256, geometry=True)[2]
    deep, top = geo(max(H >> 3, 1), max(W >> 3, 1)), geo(H, W)
    tb = deep["TB"]
    rows = sorted({0, 1, tb - 1, tb, bsz // 3, bsz // 2 + 3, bsz - 2, bsz - 1})
    assert tb >= 8 and len(rows) == 8 and bsz % tb == 0, (deep, rows)
    per = top["mtiles"] * top["TB"] // bsz                                  # level-0 tiles per sample (or 1 when a tile holds several)
    first_split = {(r // top["TB"]) * max(per, 1) % top["nsplit"] for r in rows}
    assert top["mtiles"] > top["nsplit"] and len(first_split) >= 4, (top, first_split)
    return rows, deep, top


def run_train_case(cid):
    from flocoder_amd._ops import fetch_tap_rows
    from flocoder_amd import _binding as B
    tag, seed, bsz, H, W, cond_kind, variant = TRAIN_CASES[cid]
    sd = synth_state_dict(load_golden("g3_unet_" + tag)["shapes"], seed)
    meta = fo.unet_meta(sd)
    model = _model(sd, mask_cond=variant == "mask")
    rows, deep, top = subset_rows(bsz, H, W)
    S = torch.tensor(rows)
    Sd = S.to(DEV)
    n = len(rows)
    g = torch.Generator().manual_seed(2000 + seed)
    x = synth_input(f"bp.{cid}", (bsz, 4, H, W), seed)                     # dense: every row is a real input
    t = torch.rand(bsz, generator=g) * 999
    cls = torch.randint(0, meta["n_classes"], (bsz,), generator=g) if cond_kind == "class" else None
    mask = (torch.rand(bsz, 4, H, W, generator=g) > 0.35).float() if variant == "mask" else None
    xd, td = x.to(DEV), t.to(DEV)
    cd = None if cls is None else cls.to(DEV)
    md = None if mask is None else mask.to(DEV)
    out = model._forward_native(xd, td, cd, md, train=True)
    d_sub = synth_input(f"bp.d.{cid}", (n, 4, H, W), seed) * torch.logspace(2, -2, n).view(n, 1, 1, 1)
    d_out = torch.zeros(bsz, 4, H, W)
    d_out[S] = d_sub                                                       # exactly zero on every other row
    flat, dx, dm = model.backward_native(xd, td, cd, d_out.to(DEV), mask=md, want_dx=True, want_dmask=True)
    torch.cuda.synchronize()
    rb, rh, rw = C.c_int(), C.c_int(), C.c_int()
    B.check(B.lib().fc_unet_reserved(model._handle, C.byref(rb), C.byref(rh), C.byref(rw)))
    mods = ut.modules(sd, masked=mask is not None)
    names = [m.name for m in mods][:-1]
    internal = [k for m in ut.modules(sd) if m.name in names for k in (m.name + s for s in m.internal)]
    got = {k: fetch_tap_rows(model, k, bsz, Sd).cpu() for k in names + internal}
    leaks = []
    rest = torch.ones(bsz, dtype=torch.bool, device=DEV)
    rest[Sd] = False
    for k in names:
        sel, leak = fetch_tap_rows(model, "grad:" + k, bsz, Sd, rest_any=True)
        got["grad:" + k] = sel.cpu()
        if leak:
            leaks.append("grad:" + k)
    for k, v in (("dx", dx), ("dmask", dm)):
        if v is not None and bool(v[rest].any()):
            leaks.append(k)
    got["x"], got["out"], got["dx"] = x[S], out[Sd].cpu(), dx[Sd].cpu()
    if dm is not None:
        got["dmask"] = dm[Sd].cpu()
    pgrads = {k: v.cpu() for k, v in model.grad_views(flat).items()}
    L = meta["n_levels"]
    forms = backward_forms(model, H, W, L)
    fwd_names, bwd_names = plan_launch_names(model)

    sd64 = {k: v.double() for k, v in sd.items()}
    ts, cs = t[S], None if cls is None else cls[S]
    cond = {} if cs is None else {"class_cond": cs}
    if mask is not None:
        cond["mask_cond"] = mask[S]
    temb = ut.conditioning(sd, ts, cond or None)
    m64 = ut.mask_of(sd, cond)
    frows = ut.gate(sd64, got, ut.local_references(sd64, temb, got, m64, internal=True), masked=m64 is not None)
    refs = gt.local_vjp(sd64, temb, got, gt.cotangents(sd64, got, d_sub, masked=m64 is not None), ts.double(), cs, m64)
    grows, prows = gt.gate_activations(got, refs), gt.gate_params(pgrads, refs)
    return dict(frows=frows, grows=grows, prows=prows, forms=forms, reserved=rb.value, refs=refs, pgrads=pgrads, rows=rows, deep=deep, top=top,
                leaks=leaks, fwd_names=fwd_names, bwd_names=bwd_names)


@pytest.mark.parametrize("cid", [_heavy(c) for c in TRAIN_CASES])
def test_training_batch_plan_matches_its_fp64_local_vjp_on_a_sparse_cotangent(cid):
    """The backward is linear in the output cotangent: with d_out non-zero on 8 rows only, the fp64 local VJP of those 8 rows (summed for the
    parameters) is the reference of the whole 256- or 2048-row step, at the gates of the small cases, and every other row's activation
    gradient must be zero to the bit -- the check that no sample's gradient leaks into a tile mate's in the multi-sample tiles."""
    r = run_train_case(cid)
    bsz, variant = TRAIN_CASES[cid][2], TRAIN_CASES[cid][6]
    print(f"\n[{cid}] B={bsz}, cotangent on rows {r['rows']}; deepest level {r['deep']}, level 0 {r['top']}\n  forward {ut.report(r['frows'])}\n"
          f"  backward {len(r['grows'])} (tap, sample) rows, {len(r['prows'])} parameters; {gt.report(r['grows'], r['prows'])}")
    for what, names in (("forward-train", r["fwd_names"]), ("backward", r["bwd_names"])):
        uniq = sorted(set(names))
        print(f"  {what} plan: {len(names)} launches, {len(uniq)} forms: " + ", ".join(f"{k} x{names.count(k)}" for k in uniq))
    assert r["reserved"] == bsz, r["reserved"]            # the plan gated is the training plan of this batch, not a smaller one
    assert all(row.ok for row in r["frows"]), f"{cid}: forward taps: {ut.report(r['frows'])}"
    kernels = {k for k, _ in r["forms"]}
    assert kernels <= BACKWARD_KERNELS, f"{cid}: backward launch forms without a parity case: {sorted(kernels - BACKWARD_KERNELS)}"
    assert {"conv_wgrad_table", "wgrad_reduce", "finalize_table"} <= kernels
    taps = {row.tap for row in r["grows"]}
    assert {"dx", "grad:init", "grad:mid_attn", "grad:final_res_block"} <= taps and len({row.sample for row in r["grows"]}) == len(r["rows"])
    if variant == "mask":
        assert "dmask" in taps and r["refs"].params["mask_fusion_conv.0.weight"] is not None
    assert not r["leaks"], f"{cid}: rows without a cotangent have a non-zero gradient in {r['leaks']}"
    assert all(row.ok for row in r["grows"]) and all(row.ok for row in r["prows"]), f"{cid}: {gt.report(r['grows'], r['prows'])}"


@pytest.mark.timeout(600)
def test_the_cases_cover_every_backward_kernel():
    """A planner change that moves a module to another backward launch form must not silently drop that form from these gates."""
    for cid in CASES:
        if cid not in _SEEN:                            # (this test run on its own)
            run_case(cid)
    seen = set().union(*_SEEN.values())
    print(f"\nbackward launch forms gated: {sorted(seen)}")
    assert BACKWARD_KERNELS <= seen, f"no case runs {sorted(BACKWARD_KERNELS - seen)}"
    assert seen <= BACKWARD_KERNELS, f"backward launch forms without a parity case: {sorted(seen - BACKWARD_KERNELS)}"
