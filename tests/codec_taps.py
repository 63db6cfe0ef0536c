"""Module-local fp64 references for the taps of the two codecs' plans, and the per-sample gates on them (test helper, imported by
tests/test_gpu_codec_module_parity.py and tests/test_codec_taps_cpu.py; not a conftest).  The codecs' counterpart of tests/unet_taps.py.

With ``debug_taps(True)`` a codec's plans recycle no buffer and name every module's tensors (``fc_vae_debug_tensor`` /
``fc_vqvae_debug_tensor``, read with ``_ops.fetch_tap(codec, name, B, decode)``): the SD-VAE's ``conv_in``, every resnet (and its conv1
output ``.h1``), every down / upsampler, the mid attentions' ``.q .k .v .p .o`` (``.p``: the scores after the softmax), ``conv_out``,
``quant_conv`` / ``post_quant_conv``; the VQVAE's blocks by state_dict prefix with ``.h1`` (conv1), ``.act`` (its activation, where an
attention reads it), ``.mid`` (what conv2 reads), ``.h2``, ``.res`` (the downsample.0 convolution), the attentions' ``.q .k .v .p .o`` or
``.qkv .att`` (NATTEN; ``.att`` carries gamma), and the decoder's layers by ``decoder.layers.<index>`` (a convolution followed by SiLU is
kept after the SiLU, the PixelShuffle under its own index).  ``sd_modules`` / ``vq_modules`` list them in execution order, each with the
taps it reads; ``local_references`` recomputes each in fp64 from the GPU's OWN input taps with the functions of oracle/sdvae_oracle.py and
oracle/vqvae_oracle.py, so every per-sample GEMM, the softmax, a GroupNorm's eps or a stride-2 overhang answers for itself:

    module output      ||got - ref||_b <= MODULE_TOL ||ref||_b                                   per sample b
    residual branch    ||got - ref||_b <= BRANCH_TOL ||ref - x||_b + STORE_FLOOR ||got||_b         identity-residual modules

with the U-Net's numbers (unet_taps.py: MODULE_TOL 2e-6, BRANCH_TOL 3e-6, STORE_FLOOR 2^-22).  A tap class's gate is raised only against
the reference: ``e32`` evaluates every local reference in fp32 on the CPU, and a class may go up to 8 x its worst fp32 error (the MFMA's
k-ordered chain against the CPU's blocked sums); such classes are listed in CLASS_TOL with their figures.  Split-bf16 plans are gated at
the per-convolution bound of tests/test_gpu_conv.py::test_conv_split_bf16 (SPLIT_TOL = 2e-5, 2^-16 per product), module gate only.

Measured on one MI355X (tests/test_gpu_codec_module_parity.py -s prints them), worst module / worst branch error per case:

    case                              worst module                       worst branch
    sd-enc-B2-64                      6.7e-7 (mid attention .p)          6.2e-7 (down_blocks.1.resnets.1)
    sd-enc-B1-64x128                  6.5e-7 (mid attention .p)          6.2e-7
    sd-dec-B3-8x8                     8.7e-7 (up_blocks.3.resnets.0.h1)  6.5e-7 (up_blocks.3.resnets.1)
    sd-dec-B1-16x8                    8.6e-7                             6.5e-7
    sd-dec-B1-32x32-M256              2.6e-6 (.p at n = 1024, CLASS_TOL; every other class <= 8.6e-7)   6.5e-7
    sd-dec-B2-8x8-bf16x3              4.6e-6 (split resnets; SPLIT_TOL)  4.5e-6 (reported, not gated)
    sd-dec-B1-32x32-M256-bf16x3       4.5e-6                             4.5e-6 (reported, not gated)
    vq-gray-enc-B3-64x128             4.1e-7 (encoder.8.h1)              -
    vq-gray-dec-B3-4x8                4.2e-7 (decoder.layers.7)          2.1e-7 (rope_attn)
    vq-gray-dec-B2-16x32              9.7e-7 (decoder.layers.7)          2.7e-7 (rope_attn)
    vq-gray-dec-B96-8x8-M64N64        8.3e-7 (decoder.layers.6.h1)       3.1e-7 (decoder.layers.6.mid)
    vq-midi-enc-B8-128-M256           8.5e-7 (encoder.1.h2)              -
    vq-midi-enc-B8-128-M256-bf16x3    4.6e-6                             -
    vq-natten-L1 / -L2                3.3e-7 / 3.1e-7                    1.1e-7 / 1.2e-7 (NATTEN block)
    vq-natten-L1-dec / -L2-dec        4.4e-7 / 4.4e-7                    1.1e-7 / 1.2e-7

The fp32 CPU evaluation (e32) of the same references sits at 0.4-3e-7 per class, 6.5e-7 to 1.1e-6 for ``.p``.  Keep-all mode is for tests:
one 256x256 SD-VAE decode (B = 1) holds 908 MiB of activations against 348 MiB of the recycled plan.
"""
from __future__ import annotations

from typing import Callable, Dict, List, NamedTuple, Optional, Sequence

import torch
import torch.nn.functional as F

from oracle import sdvae_oracle as vo
from oracle import vqvae_oracle as vq
from unet_taps import BRANCH_TOL, MODULE_TOL, STORE_FLOOR, Row, report  # noqa: F401  (re-exported)

SPLIT_TOL = 2e-5
# tap class -> (module gate, branch gate) where the U-Net's numbers do not hold; each entry states the class's worst fp32-CPU error (e32)
CLASS_TOL: Dict[str, tuple] = {
    # softmax(q k^T / sqrt(C)) from the GPU's q and k: an absolute error in a logit is a relative error in its probability, and a logit
    # is a C = 512-term fp32 dot product whose terms cancel.  At n = 1024 (sd-dec-B1-32x32-M256) the fp32 CPU evaluation of the same
    # reference is off by 1.1e-6 (e32) and the GPU by 2.6e-6; at n <= 128 both sit at 6-9e-7.  4.5 x e32, inside the 8 x allowed.
    "attn.p": (5e-6, BRANCH_TOL),
}


class Module(NamedTuple):
    name: str                       # the tap it produces ("out": the codec's output)
    inputs: Sequence[str]           # taps it reads ("x": the codec's input)
    fn: Callable                    # fn(sd, *inputs) -> tensor
    residual: Optional[str]         # the input tap added back unchanged (identity residual), else None
    cls: str                        # tap class: the rows that share a gate and a line of the report


def _attention(mods: List[Module], orc, a: str, tap: str, src: str, close: Callable, out: str):
    """q / k / v from ``src``; the scores from the GPU's q and k; p v from the GPU's p and v; the projection and residual from its o."""
    for i, u in enumerate("qkv"):
        mods.append(Module(f"{tap}.{u}", (src,), lambda sd, x, i=i: orc.attn_qkv(sd, a, x)[i], None, "attn.qkv"))
    mods.append(Module(tap + ".p", (tap + ".q", tap + ".k"), lambda sd, q, k: orc.attn_probs(q, k), None, "attn.p"))
    mods.append(Module(tap + ".o", (tap + ".p", tap + ".v"), lambda sd, p, v: orc.attn_apply(p, v), None, "attn.o"))
    mods.append(Module(out, (tap + ".o", src), lambda sd, o, x: close(sd, a, o, x), src, "attn"))


# ---- SD-VAE ------------------------------------------------------------------------------------------------------------------------
def sd_modules(sd, decode: bool) -> List[Module]:
    mods: List[Module] = []

    def one(name, src, fn, cls):
        mods.append(Module(name, (src,), fn, None, cls))
        return name

    def resnet(n, src):
        mods.append(Module(n + ".h1", (src,), lambda sd, x: vo.resnet_h1(sd, n, x), None, "resnet.h1"))
        ident = (n + ".conv_shortcut.weight") not in sd
        mods.append(Module(n, (src, n + ".h1"), lambda sd, x, h1: vo.resnet_close(sd, n, x, h1), src if ident else None, "resnet"))
        return n

    def mid(n, src):
        src = resnet(n + ".resnets.0", src)
        a = n + ".attentions.0"
        _attention(mods, vo, a, a, src, vo.attn_close, a)
        return resnet(n + ".resnets.1", a)

    def blocks(prefix):
        return 1 + max(int(k.split(".")[2]) for k in sd if k.startswith(prefix))

    if not decode:
        h = one("encoder.conv_in", "x", lambda sd, x: vo._conv(sd, "encoder.conv_in", x, padding=1), "conv_in")
        for i in range(blocks("encoder.down_blocks.")):
            j = 0
            while f"encoder.down_blocks.{i}.resnets.{j}.norm1.weight" in sd:
                h = resnet(f"encoder.down_blocks.{i}.resnets.{j}", h); j += 1
            d = f"encoder.down_blocks.{i}.downsamplers.0"
            if d + ".conv.weight" in sd:
                h = one(d, h, lambda sd, x, d=d: vo.downsample(sd, d, x), "downsample")
        h = mid("encoder.mid_block", h)
        h = one("encoder.conv_out", h, lambda sd, x: vo.conv_out(sd, "encoder", x), "conv_out")
        h = one("quant_conv", h, lambda sd, x: vo._conv(sd, "quant_conv", x), "quant_conv")
        one("out", h, lambda sd, m: m[:, : m.shape[1] // 2], "out")
        return mods
    h = one("post_quant_conv", "x", lambda sd, x: vo._conv(sd, "post_quant_conv", x), "quant_conv")
    h = one("decoder.conv_in", h, lambda sd, x: vo._conv(sd, "decoder.conv_in", x, padding=1), "conv_in")
    h = mid("decoder.mid_block", h)
    for i in range(blocks("decoder.up_blocks.")):
        j = 0
        while f"decoder.up_blocks.{i}.resnets.{j}.norm1.weight" in sd:
            h = resnet(f"decoder.up_blocks.{i}.resnets.{j}", h); j += 1
        u = f"decoder.up_blocks.{i}.upsamplers.0"
        if u + ".conv.weight" in sd:
            h = one(u, h, lambda sd, x, u=u: vo.upsample(sd, u, x), "upsample")
    h = one("decoder.conv_out", h, lambda sd, x: vo.conv_out(sd, "decoder", x), "conv_out")
    one("out", h, lambda sd, y: y[:, : sd["decoder.conv_out.weight"].shape[0]], "out")     # the tap pads RGB to 4 channels
    return mods


def sharpen(sd: Dict[str, torch.Tensor], gain: float = 2.0) -> Dict[str, torch.Tensor]:
    """``sd`` with the attentions' to_q / to_k weights times ``gain``.  At He-scaled random weights some softmax rows are nearly flat
    (logit standard deviation down to 0.43); doubling both gives 1.7, so a wrong scale shows."""
    return {k: v * gain if k.endswith((".to_q.weight", ".to_k.weight")) else v for k, v in sd.items()}


def sdvae_weights(shapes: Dict[str, tuple], seed: int) -> Dict[str, torch.Tensor]:
    """Seeded random SD-VAE weights over a shape table by SD_VAE_Wrapper's recipe (norms 1 + 0.1 n / biases 0.05 n / He-scaled
    matrices), sharpened -- for tests that run without the library."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in shapes.items():
        if len(shape) == 1:
            sd[name] = 1.0 + 0.1 * torch.randn(shape, generator=g) if name.endswith(".weight") else 0.05 * torch.randn(shape, generator=g)
        else:
            sd[name] = torch.randn(shape, generator=g) * (1.0 / torch.Size(shape[1:]).numel()) ** 0.5
    return sharpen(sd)


def min_logit_std(q: torch.Tensor, k: torch.Tensor) -> float:
    """The smallest standard deviation, over the keys, of any query's logits q k^T / sqrt(C) (NCHW q, k): a softmax whose rows are nearly
    flat hides a wrong scale."""
    b, c, h, w = q.shape
    s = torch.bmm(q.reshape(b, c, h * w).permute(0, 2, 1), k.reshape(b, c, h * w)) * c ** -0.5
    return float(s.std(dim=2).min())


# ---- VQVAE -------------------------------------------------------------------------------------------------------------------------
def vq_modules(sd, decode: bool, layout: int = 1) -> List[Module]:
    mods: List[Module] = []

    def one(name, src, fn, cls, residual=None):
        mods.append(Module(name, (src,), fn, residual, cls))
        return name

    def block(n, src, stride=1):
        one(n + ".h1", src, lambda sd, x: vq._conv(sd, n + ".conv1", x, padding=1, stride=stride), "block.h1")
        a = n + ".attn"
        if (a + ".q.weight") in sd or (a + ".qkv.weight") in sd:
            one(n + ".act", n + ".h1", lambda sd, h1: vq.block_act(sd, n, h1), "block.act")
        if (a + ".q.weight") in sd:
            _attention(mods, vq, a, n, n + ".act", lambda sd, a, o, x: x + vq._conv(sd, a + ".proj_out", o), n + ".mid")
        elif (a + ".qkv.weight") in sd:
            one(n + ".qkv", n + ".act", lambda sd, x: vq.natten_qkv(sd, a, x), "natten.qkv")
            one(n + ".att", n + ".qkv", lambda sd, t: vq.natten_att(t, layout) * sd[a + ".gamma"], "natten.att")
            mods.append(Module(n + ".mid", (n + ".att", n + ".act"),
                               lambda sd, t, x: x + F.linear(t.permute(0, 2, 3, 1), sd[a + ".proj.weight"]).permute(0, 3, 1, 2), n + ".act", "natten"))
        else:
            one(n + ".mid", n + ".h1", lambda sd, h1: vq.block_act(sd, n, h1), "block.act")
        one(n + ".h2", n + ".mid", lambda sd, m: vq._conv(sd, n + ".conv2", m, padding=1), "block.h2")
        if (n + ".downsample.0.weight") in sd:
            one(n + ".res", src, lambda sd, x: vq._conv(sd, n + ".downsample.0", x, stride=stride), "block.res")
            mods.append(Module(n, (n + ".h2", src, n + ".res"), lambda sd, h2, x, r: vq.block_close(sd, n, h2, x, r), None, "block"))
        else:
            mods.append(Module(n, (n + ".h2", src), lambda sd, h2, x: vq.block_close(sd, n, h2, x), None, "block"))
        return n

    nd = vq.n_downsamples(sd)
    if not decode:
        h = "x"
        for i in range(nd):
            h = block(f"encoder.{2 * i}", h, 2)
            h = block(f"encoder.{2 * i + 1}", h)
        h = block(f"encoder.{2 * nd}", h)
        for j in (1, 2):
            h = one(f"encoder.{2 * nd + j}", h, lambda sd, x, j=j: vq._conv(sd, f"encoder.{2 * nd + j}", x), "compress")
        h = one(f"encoder.{2 * nd + 5}", h, lambda sd, x: vq.compress_out(sd, nd, x), "compress")
        one("out", h, lambda sd, y: y, "out")
        return mods
    L = "decoder.layers."
    h, i = "x", 0
    if (L + "0.q_proj.weight") in sd:
        h = one(L + "0", "x", lambda sd, x: vq.spatial_nonlocal_attention(sd, L + "0", x), "rope_attn", residual="x"); i = 1
    emb = sd[L + str(i) + ".weight"].shape[1]
    h = one(L + str(i), h, lambda sd, x, i=i: vq._conv(sd, L + str(i), x), "expand")
    h = one(L + str(i + 3), h, lambda sd, x, i=i: vq.expand_out(sd, i, x, emb), "expand")
    h = block(L + str(i + 5), h)
    i += 6
    for _ in range(nd):
        h = one(L + str(i), h, lambda sd, x, i=i: F.silu(vq._conv(sd, L + str(i), x, padding=1)), "up.conv")
        h = one(L + str(i + 2), h, lambda sd, x: F.pixel_shuffle(x, 2), "pixel_shuffle")
        h = block(L + str(i + 4), h)
        h = block(L + str(i + 6), h)
        i += 7
    h = one(L + str(i + 1), h, lambda sd, x, i=i: F.silu(vq._conv(sd, L + str(i + 1), x, padding=1)), "final")
    h = one(L + str(i + 4), h, lambda sd, x, i=i: vq._conv(sd, L + str(i + 4), x, padding=1), "final")
    one("out", h, lambda sd, y, i=i: y[:, : sd[L + str(i + 4) + ".weight"].shape[0]], "out")    # the tap pads the channels to 4
    return mods


# ---- references and gates --------------------------------------------------------------------------------------------------------------
def needed_taps(mods: Sequence[Module], only: Optional[Callable] = None) -> List[str]:
    """The taps to fetch for ``mods`` (restricted to the modules ``only(name)`` keeps): their outputs and inputs, without "x" / "out"."""
    keep = [m for m in mods if only is None or only(m.name)]
    names = {m.name for m in keep} | {n for m in keep for n in m.inputs}
    return [m.name for m in mods if m.name in names and m.name != "out"]


def local_references(sd64: Dict[str, torch.Tensor], got: Dict[str, torch.Tensor], mods: Sequence[Module], only: Optional[Callable] = None,
                     dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """The reference of every module's output, each computed from the taps in ``got`` -- the GPU's -- that the module reads.  ``got``
    holds "x" (the codec's input), "out" and the taps; a tap with channels padded to 4 is cut to what its reader's weights take.
    ``dtype`` float32: the same evaluation in fp32 on fp32 weights (``e32``)."""
    sd = sd64 if dtype == torch.float64 else {k: v.to(dtype) for k, v in sd64.items()}
    refs: Dict[str, torch.Tensor] = {}
    with torch.no_grad():
        for mod in mods:
            if only is not None and not only(mod.name):
                continue
            refs[mod.name] = mod.fn(sd, *[got[n].detach().to(dtype).cpu() for n in mod.inputs])
    return refs


def _cut(g: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """A tap whose channels the library pads to a multiple of 4 (RGB / gray ends): the padding holds zeros and is not part of the tensor."""
    if g.shape[1] != ref.shape[1]:
        assert g.shape[1] == (ref.shape[1] + 3) // 4 * 4 and not g[:, ref.shape[1]:].any(), (tuple(g.shape), tuple(ref.shape))
        g = g[:, : ref.shape[1]]
    return g


def gate(mods: Sequence[Module], got: Dict[str, torch.Tensor], refs: Dict[str, torch.Tensor], module_tol: Optional[float] = None,
         branch_tol: Optional[float] = None, branch: bool = True) -> List[Row]:
    """Per-sample rows (tap, sample, module error, branch error, ok) for every tap in ``refs``.  The gates are CLASS_TOL's for the tap's
    class, else MODULE_TOL / BRANCH_TOL; ``module_tol`` / ``branch_tol`` replace them for all classes (split-bf16: ``branch`` off)."""
    by_name = {m.name: m for m in mods}
    rows: List[Row] = []
    for name, ref in refs.items():
        mod = by_name[name]
        ref = ref.double()
        g = _cut(got[name].double().cpu(), ref)
        assert g.shape == ref.shape, (name, tuple(g.shape), tuple(ref.shape))
        mt, bt = CLASS_TOL.get(mod.cls, (MODULE_TOL, BRANCH_TOL))
        mt, bt = module_tol or mt, branch_tol or bt
        d = (g - ref).flatten(1).norm(dim=1)
        rn = ref.flatten(1).norm(dim=1).clamp_min(1e-30)
        if mod.residual is not None:
            br = (ref - _cut(got[mod.residual].double().cpu(), ref)).flatten(1).norm(dim=1).clamp_min(1e-30)
            bound = bt * br + STORE_FLOOR * g.flatten(1).norm(dim=1)
        for b in range(ref.shape[0]):
            ok = bool(d[b] <= mt * rn[b])
            be = float("nan")
            if mod.residual is not None:
                be = float(d[b] / br[b])
                if branch:
                    ok = ok and bool(d[b] <= bound[b])
            rows.append(Row(name, b, float(d[b] / rn[b]), be, ok))
    return rows


def e32(sd64, got, mods: Sequence[Module], only: Optional[Callable] = None, refs64=None) -> Dict[str, tuple]:
    """tap class -> (worst module error, worst branch error) of the fp32 CPU evaluation of the local references against the fp64 one,
    from the same input taps: what fp32 arithmetic costs this class on this data, independent of the kernels."""
    refs64 = refs64 if refs64 is not None else local_references(sd64, got, mods, only)
    refs32 = local_references(sd64, got, mods, only, dtype=torch.float32)
    by_name = {m.name: m for m in mods}
    worst: Dict[str, list] = {}
    for name, r64 in refs64.items():
        mod = by_name[name]
        d = (refs32[name].double() - r64).flatten(1).norm(dim=1)
        m = float((d / r64.flatten(1).norm(dim=1).clamp_min(1e-30)).max())
        b = float("nan")
        if mod.residual is not None:
            b = float((d / (r64 - _cut(got[mod.residual].double().cpu(), r64)).flatten(1).norm(dim=1).clamp_min(1e-30)).max())
        w = worst.setdefault(mod.cls, [0.0, float("nan")])
        w[0] = max(w[0], m)
        if b == b:
            w[1] = b if w[1] != w[1] else max(w[1], b)
    return {k: tuple(v) for k, v in worst.items()}


def by_class(mods: Sequence[Module], rows: Sequence[Row]) -> Dict[str, tuple]:
    """tap class -> (worst module error, worst branch error) over ``rows``."""
    cls = {m.name: m.cls for m in mods}
    out: Dict[str, list] = {}
    for r in rows:
        w = out.setdefault(cls[r.tap], [0.0, float("nan")])
        w[0] = max(w[0], r.module)
        if r.branch == r.branch:
            w[1] = r.branch if w[1] != w[1] else max(w[1], r.branch)
    return {k: tuple(v) for k, v in out.items()}
