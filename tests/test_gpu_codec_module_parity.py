"""Every tapped module of the two codecs (SD-VAE csrc/vae.hip, VQVAE csrc/vqvae.hip), per sample, against an fp64 reference computed
from the GPU's own input taps (tests/codec_taps.py; the gates are documented there).  The whole-image rel-L2 of tests/test_gpu_vae.py /
test_gpu_vqvae.py / test_gpu_natten.py dilutes a module's error by the rest of the codec and a sample's by its batch mates, and sits
10-100x above what fp32 needs; here each (tap, sample) answers for itself:

    module output   rel-L2 <= 2e-6 per sample
    residual branch ||out - ref|| <= 3e-6 ||ref - x|| + 2^-22 ||out||  per sample (identity resnets, attentions, rope_attn)

(measured on one MI355X: worst module 9.7e-7, worst branch 6.5e-7; the scores after a 1024-column softmax 2.6e-6 against a class gate of
5e-6, codec_taps.CLASS_TOL; split-bf16 plans 4.6e-6 against the per-convolution 2e-5).

The cases together put every launch form the codec builders can emit on the path: each names the launches it exists for and asserts
them from the plan, and the coverage test asserts that the union equals CODEC_KERNELS.  With -s every case prints its worst errors."""
import pytest
import torch

import codec_taps as ct
from conftest import load_golden
from oracle.synth import synth_state_dict, synth_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M256 = "conv_igemm<M256,N64>"
M64N64 = "conv_igemm<M64,N64,K2>"
SPLIT_TILES = ("conv_igemm<M128,N32>", "conv_igemm<M128,N64>", M256)       # the tiles that have a split-bf16 instantiation

# every launch name a codec plan can hold (templates kept: the tile is the point); "@bf16x3": a tile with a split-bf16 instantiation in
# a plan built at set_precision("bf16x3") (its shared-weight 1x1 / 3x3 / folded-upsampling launches run split, conv_igemm.hip `bf3`)
CODEC_KERNELS = {"nchw_to_nhwc", "nhwc_to_nchw", "finalize", "gn_stats", "gn_fold", "transpose", "softmax_rows", "rope_attn", "na2d",
                 "pixel_shuffle", "conv_igemm<M128,N32>", "conv_igemm<M128,N64>", "conv_igemm<M64,N32,K2>", "conv_igemm<M32,N32,K4>",
                 M64N64, M256, *(t + "@bf16x3" for t in SPLIT_TILES)}

VQ_CFG = {"midi_vqgan": dict(in_channels=3, hidden_channels=256, num_downsamples=3, internal_dim=128, vq_embedding_dim=4),
          "gray_nd4_small": dict(in_channels=1, hidden_channels=32, num_downsamples=4, internal_dim=32, vq_embedding_dim=4)}
ATTN = ("transpose", "softmax_rows")

# id: (codec, decode, input shape, precision, the modules gated (name prefixes; None: all), launches the case exists for)
CASES = {
    "sd-enc-B2-64": ("sd", False, (2, 3, 64, 64), "fp32", None, {*ATTN, "finalize", "gn_fold"}),
    "sd-enc-B1-64x128": ("sd", False, (1, 3, 64, 128), "fp32", None, {*ATTN}),
    "sd-dec-B3-8x8": ("sd", True, (3, 4, 8, 8), "fp32", None, {*ATTN, "finalize"}),
    "sd-dec-B1-16x8": ("sd", True, (1, 4, 16, 8), "fp32", None, {*ATTN}),
    "sd-dec-B1-32x32-M256": ("sd", True, (1, 4, 32, 32), "fp32",
                             ("decoder.mid_block.attentions.0", "decoder.up_blocks.3", "decoder.conv_out"), {*ATTN, M256, "gn_fold"}),
    "sd-dec-B2-8x8-bf16x3": ("sd", True, (2, 4, 8, 8), "bf16x3", None, {"conv_igemm<M128,N32>@bf16x3"}),
    "sd-dec-B1-32x32-M256-bf16x3": ("sd", True, (1, 4, 32, 32), "bf16x3",
                                    ("decoder.mid_block.attentions.0", "decoder.up_blocks.3", "decoder.conv_out"), {*ATTN, M256 + "@bf16x3"}),
    "vq-gray-enc-B3-64x128": ("vq-gray", False, (3, 1, 64, 128), "fp32", None, {"finalize"}),
    "vq-gray-dec-B3-4x8": ("vq-gray", True, (3, 4, 4, 8), "fp32", None, {*ATTN, "rope_attn", "pixel_shuffle", "gn_stats"}),
    "vq-gray-dec-B2-16x32": ("vq-gray", True, (2, 4, 16, 32), "fp32", None, {*ATTN, "rope_attn", "pixel_shuffle"}),
    # n = 64 tokens is fewer than the 128-row tiles take for a per-sample-weight GEMM: at B = 96 the P.V product (256 columns) fills M64N64K2
    "vq-gray-dec-B96-8x8-M64N64": ("vq-gray", True, (96, 4, 8, 8), "fp32", ("decoder.layers.6",), {M64N64}),
    "vq-midi-enc-B8-128-M256": ("vq-midi", False, (8, 3, 128, 128), "fp32", ("encoder.0", "encoder.1"), {M256}),
    "vq-midi-enc-B8-128-M256-bf16x3": ("vq-midi", False, (8, 3, 128, 128), "bf16x3", ("encoder.0", "encoder.1"),
                                       {M256 + "@bf16x3", "conv_igemm<M128,N64>@bf16x3"}),
    "vq-natten-L1": ("vq-natten-1", False, (2, 1, 128, 128), "fp32", None, {"na2d", "gn_stats"}),
    "vq-natten-L2": ("vq-natten-2", False, (2, 1, 128, 128), "fp32", None, {"na2d", "gn_stats"}),
    "vq-natten-L1-dec": ("vq-natten-1", True, (2, 4, 16, 16), "fp32", None, {"na2d", "pixel_shuffle"}),
    "vq-natten-L2-dec": ("vq-natten-2", True, (2, 4, 16, 16), "fp32", None, {"na2d", "pixel_shuffle"}),
}
_CODECS, _SEEN = {}, {}


def _codec(kind):
    """(codec on the GPU, its fp64 state dict, NATTEN layout), built once per kind."""
    if kind in _CODECS:
        return _CODECS[kind]
    from flocoder_amd.codecs import SD_VAE_Wrapper, VQVAE
    layout = 1
    if kind == "sd":                                  # the wrapper's seeded random table with to_q / to_k doubled (codec_taps.sharpen)
        m = SD_VAE_Wrapper(weights="random", seed=7).eval()
        sd = ct.sharpen({k[4:]: v.detach().clone() for k, v in m.state_dict().items()})
        m.load_vae_state_dict(sd)
    elif kind.startswith("vq-natten"):                # the configuration of tests/test_gpu_natten.py, gates open
        layout = int(kind[-1])
        m = VQVAE(natten_layout=layout, in_channels=1, hidden_channels=32, num_downsamples=3, internal_dim=32, vq_embedding_dim=4,
                  decoder_nonlocal=False).eval()
        own = {k: v for k, v in m.state_dict().items() if k != "codebook_usage" and not k.startswith("vq.") and "noise" not in k.lower()}
        sd = {k: synth_tensor(k, v.shape, 4) for k, v in own.items()}
        for k in own:
            if k.endswith(".attn.gamma"):
                sd[k] = torch.tensor([0.8])
            elif k.endswith((".attn.qkv.weight", ".attn.proj.weight")):
                sd[k] = sd[k] * 1.5
        m.load_state_dict(sd, strict=False)
    else:
        tag = {"vq-gray": "gray_nd4_small", "vq-midi": "midi_vqgan"}[kind]
        sd = synth_state_dict(load_golden("g9_vqvae")[tag + "_shapes"], 9)
        m = VQVAE(**VQ_CFG[tag]).eval()
        m.load_state_dict(sd, strict=False)
    _CODECS[kind] = (m.to(DEV), {k: v.double() for k, v in sd.items()}, layout)
    return _CODECS[kind]


def _under(name, prefixes):
    """``name`` is one of the modules ``prefixes`` (None: all) or a tap inside one."""
    return prefixes is None or name == "out" or any(name == p or name.startswith(p + ".") for p in prefixes)


def _input(cid, kind, decode, shape):
    g = torch.Generator().manual_seed(sum(map(ord, cid)))
    if decode:
        return torch.randn(shape, generator=g) * (4.5 if kind == "sd" else 1.0)      # unscaled SD latents
    x = torch.rand(shape, generator=g)
    return x * 2 - 1 if kind == "sd" else x


def run_case(cid):
    """-> (module list, the GPU's taps, fp64 local references, gate rows, launches (kernel, module) of the plan)."""
    from flocoder_amd._ops import fetch_tap
    kind, decode, shape, prec, prefixes, _ = CASES[cid]
    codec, sd64, layout = _codec(kind)
    mods = ct.sd_modules(sd64, decode) if kind == "sd" else ct.vq_modules(sd64, decode, layout)
    only = None if prefixes is None else (lambda n: _under(n, prefixes))
    x = _input(cid, kind, decode, shape)
    codec.set_precision(prec)
    codec.debug_taps(True)
    try:
        out = (codec.decode if decode else codec.encode)(x.to(DEV))
        got = {n: fetch_tap(codec, n, shape[0], decode).cpu() for n in ct.needed_taps(mods, only)}
        ops = [(k + "@bf16x3" if prec == "bf16x3" and k in SPLIT_TILES else k, m) for k, m, _ in codec.plan_ops(decode)]
    finally:
        codec.debug_taps(False)
        codec.set_precision("fp32")
    got["x"], got["out"] = x, out.cpu()
    _SEEN[cid] = {k for k, m in ops if _under(m, prefixes) or m in ("input", "sample", "recon", "z", "latent_dist.mean")}   # gated launches only
    refs = ct.local_references(sd64, got, mods, only)
    split = prec == "bf16x3"
    rows = ct.gate(mods, got, refs, module_tol=ct.SPLIT_TOL if split else None, branch=not split)
    return mods, got, refs, rows, ops


def describe(cid, mods, rows):
    cls = ct.by_class(mods, rows)
    return (f"[{cid}] {len(rows)} (tap, sample) rows; {ct.report(rows)}\n    by class (module/branch): "
            + ", ".join(f"{k} {m:.1e}/{b:.1e}" for k, (m, b) in sorted(cls.items())))


@pytest.mark.parametrize("cid", list(CASES))
def test_every_codec_module_and_sample_matches_its_fp64_reference(cid):
    kind, decode, shape, prec, prefixes, needs = CASES[cid]
    mods, got, refs, rows, ops = run_case(cid)
    print("\n" + describe(cid, mods, rows))
    kernels = _SEEN[cid]                              # the launches of the modules this case gates
    assert needs <= kernels, f"{cid}: the gated modules no longer run {sorted(needs - kernels)}; they run {sorted(kernels)}"
    if kind == "sd":
        a = ("decoder" if decode else "encoder") + ".mid_block.attentions.0"
        assert ct.min_logit_std(refs[a + ".q"], refs[a + ".k"]) >= 1.0
    want = {m.name for m in mods if _under(m.name, prefixes)}
    by_tap = {}
    for r in rows:
        by_tap.setdefault(r.tap, set()).add(r.sample)
    assert set(by_tap) == want and all(s == set(range(shape[0])) for s in by_tap.values())      # every gated tap, every sample
    assert all(r.ok for r in rows), describe(cid, mods, rows)


def test_the_cases_cover_every_codec_launch_form():
    """A planner change that moves a codec module to another launch form must not silently drop that form from the module gate."""
    for cid in CASES:
        if cid not in _SEEN:                          # (this test run on its own)
            run_case(cid)
    seen = set().union(*_SEEN.values())
    print(f"\nlaunch forms gated: {sorted(seen)}")
    assert seen == CODEC_KERNELS, f"ungated {sorted(CODEC_KERNELS - seen)}; not listed {sorted(seen - CODEC_KERNELS)}"


@pytest.mark.parametrize("cid", ["sd-dec-B3-8x8", "vq-gray-dec-B3-4x8"])
def test_taps_change_nothing(cid):
    """Same launches and same bits with the taps on, and switching them off again restores the recycled plan."""
    kind, decode, shape, _, _, _ = CASES[cid]
    codec, _, _ = _codec(kind)
    x = _input(cid, kind, decode, shape).to(DEV)
    off = codec.decode(x)
    k_off = codec.plan_ops(True)
    with pytest.raises(ValueError, match="no tap named"):
        codec.debug_tensor(k_off[1][1], True)
    codec.debug_taps(True)
    try:
        on = codec.decode(x)
        k_on = codec.plan_ops(True)
        assert codec.debug_tensor(k_off[1][1], True)[0]
    finally:
        codec.debug_taps(False)
    again = codec.decode(x)
    assert torch.equal(on, off) and k_on == k_off and len(k_on) == codec._fn("plan_launches")(codec._handle, 1)
    assert torch.equal(again, off) and codec.plan_ops(True) == k_off
    with pytest.raises(ValueError, match="no tap named"):
        codec.debug_tensor(k_off[1][1], True)
