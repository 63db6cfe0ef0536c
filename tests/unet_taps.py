"""Module-local fp64 references for the U-Net forward's taps, and the per-sample gates on them (test helper, imported by
tests/test_gpu_unet_module_parity.py and tests/test_unet_module_parity_cpu.py; not a conftest).

The library names the output of every block of its forward plan (``fc_unet_debug_tensor``, read with ``_ops.fetch_tap``): ``init``,
``downs.i.{0,1,2,3}``, ``mid_block1``, ``mid_attn``, ``mid_block2``, ``ups.i.{0,1,2,3}``, ``final_res_block``; the training plan also
keeps the raw conv outputs ``<resblock>.h1`` / ``.h2`` and the linear attention's ``.qkv`` / ``.lao`` / ``.y``.  ``local_references``
recomputes each of them in fp64 from the GPU's OWN input taps with the oracle's module functions, so an error stays with the module that
made it instead of piling up along the network, and a gate can sit near fp32 rounding:

    module output      ||got - ref||_b <= MODULE_TOL ||ref||_b                                   per sample b
    residual branch    ||got - ref||_b <= BRANCH_TOL ||ref - x||_b + STORE_FLOOR ||got||_b         identity-residual modules

The branch gate is ``(got - x)`` against ``(ref - x)``: a module whose branch is small next to its input (a late linear attention) can be
100x worse than fp32 rounding in that branch and still sit within MODULE_TOL of its output.  STORE_FLOOR = 2^-22 is twice the unit
roundoff of fp32: storing ``got`` alone costs up to 2^-24 per element, and the GPU's ``x`` (which both sides add) is itself fp32.

The bounds are set from the MI355X: over the ~14,500 (module, sample) rows of tests/test_gpu_unet_module_parity.py the worst module
error is 5.1e-7 (a training plan's raw ups conv output) and the worst branch error 6.1e-7 (mid_block2 at C = 512), so MODULE_TOL = 2e-6
and BRANCH_TOL = 3e-6 leave a factor of 4-5 for summation order, and sit 5x and 10x below the 1e-5 / 3e-5 first proposed for them.
"""
from __future__ import annotations

from typing import Callable, Dict, List, NamedTuple, Optional, Sequence

import torch
import torch.nn.functional as F

from oracle import flow_oracle as fo

MODULE_TOL = 2e-6
BRANCH_TOL = 3e-6
STORE_FLOOR = 2.0 ** -22
INTERNAL = (".h1", ".h2", ".qkv", ".lao", ".y")


class Module(NamedTuple):
    name: str                       # the tap it produces ("out": the network output)
    inputs: Sequence[str]           # taps it reads, concatenated along channels ("x": the network input)
    fn: Callable                    # fn(ctx, x, internal) -> fp64 tensor; fills internal[<name>.<tap>] with the raw intermediate taps
    residual: Optional[str]         # the input tap added back unchanged (identity residual), else None
    internal: Sequence[str]         # intermediate tap names the training plan keeps for this module


class Ctx(NamedTuple):
    sd: Dict[str, torch.Tensor]     # fp64 state dict
    temb: torch.Tensor              # fp64 conditioning vector [B, time_dim]
    mask: Optional[torch.Tensor]    # fp64 mask_cond, or None
    groups: int


def conditioning(sd: Dict[str, torch.Tensor], time: torch.Tensor, cond: Optional[dict]) -> torch.Tensor:
    """The conditioning vector as the reference computes it -- fp32 time_mlp / class MLP on the fp32 weights -- upcast to fp64."""
    sd32 = {k: v.detach().float().cpu() for k, v in sd.items()}
    cls = cond.get("class_cond") if isinstance(cond, dict) else None
    if cls is not None:
        cls = cls.cpu()
    return fo.time_embedding(sd32, time.detach().float().cpu(), cls).double()


def mask_of(sd: Dict[str, torch.Tensor], cond: Optional[dict]) -> Optional[torch.Tensor]:
    m = cond.get("mask_cond") if isinstance(cond, dict) else None
    return m.detach().double().cpu() if (m is not None and "mask_fusion_conv.0.weight" in sd) else None


def _inject(ctx: Ctx, x, prefix, i):
    """unet.py:336-340,360-364 (the oracle's ``inject``): x + SiLU(conv3x3(cat[x, bilinear(mask)]))."""
    mr = F.interpolate(ctx.mask, size=x.shape[-2:], mode="bilinear")
    return x + F.silu(fo._conv(ctx.sd, f"{prefix}.{i}.0", torch.cat([x, mr], dim=1), padding=1))


def _init(ctx: Ctx, x, internal):
    y = fo._conv(ctx.sd, "init_conv", x)
    m = ctx.mask
    if m is not None and not torch.allclose(m, torch.ones_like(m)):       # unet.py:298-305: replaces x, no residual
        f = F.silu(fo._conv(ctx.sd, "mask_fusion_conv.0", torch.cat([y, m], dim=1), padding=2))
        f = F.silu(fo._conv(ctx.sd, "mask_fusion_conv.2", f, padding=1))
        y = fo._conv(ctx.sd, "mask_fusion_conv.4", f, padding=1)
    return y


def _resblock(p):
    def fn(ctx: Ctx, x, internal):
        taps = {}
        y = fo.resnet_block(ctx.sd, p, x, ctx.temb, ctx.groups, taps)
        internal.update(taps)
        return y
    return fn


def _linattn(p):
    def fn(ctx: Ctx, x, internal):
        sd, heads = ctx.sd, 4
        xn = fo._gn(sd, p + ".fn.norm", x, 1)                                   # the module's internals, as linear_attention computes them
        qkv = fo._conv(sd, p + ".fn.fn.to_qkv", xn)
        b, _, h, w = x.shape
        q, k, v = qkv.reshape(b, 3, heads, -1, h * w).unbind(1)
        d = q.shape[2]
        ctx_ = torch.einsum("bhdn,bhen->bhde", k.softmax(dim=-1), v)
        lao = torch.einsum("bhde,bhdn->bhen", ctx_, q.softmax(dim=-2) * d ** -0.5).reshape(b, heads * d, h, w)
        internal.update({p + ".qkv": qkv, p + ".lao": lao, p + ".y": fo._conv(sd, p + ".fn.fn.to_out.0", lao)})
        return fo._prenorm_residual(sd, p, x, fo.linear_attention)
    return fn


def _midattn(ctx: Ctx, x, internal):
    return fo._prenorm_residual(ctx.sd, "mid_attn", x, fo.full_attention)


def _down(i, last, masked):
    def fn(ctx: Ctx, x, internal):
        if masked:
            x = _inject(ctx, x, "down_mask_fusions", i)
        return fo._conv(ctx.sd, f"downs.{i}.3", x, padding=1) if last else fo.space_to_depth_conv(ctx.sd, f"downs.{i}.3.1", x)
    return fn


def _up(i, last, masked):
    def fn(ctx: Ctx, x, internal):
        if masked:
            x = _inject(ctx, x, "up_mask_fusions", i)
        if last:
            return fo._conv(ctx.sd, f"ups.{i}.3", x, padding=1)
        return fo._conv(ctx.sd, f"ups.{i}.3.1", F.interpolate(x, scale_factor=2, mode="nearest"), padding=1)   # Upsample, unet.py:42-46
    return fn


def _final(ctx: Ctx, x, internal):
    return fo._conv(ctx.sd, "final_conv", x)


def modules(sd: Dict[str, torch.Tensor], masked: bool = False) -> List[Module]:
    """The forward (unet.py:289-372) as a list of modules in execution order, each with the taps it reads: the skips are popped as the
    up path pops them, the final ResnetBlock reads the up path's output concatenated with ``init``.  ``masked``: a mask_cond is given
    (the first two levels inject it before their down / up sampling conv, oracle ``inject``)."""
    m = fo.unet_meta(sd)
    L = m["n_levels"]
    masked = masked and m["mask_cond"]
    rb = (".h1", ".h2")
    la = (".qkv", ".lao", ".y")
    out: List[Module] = [Module("init", ("x",), _init, None, ())]
    prev, skips = "init", []
    for i in range(L):
        p = f"downs.{i}"
        out.append(Module(p + ".0", (prev,), _resblock(p + ".0"), prev, rb)); skips.append(p + ".0")
        out.append(Module(p + ".1", (p + ".0",), _resblock(p + ".1"), p + ".0", rb))
        out.append(Module(p + ".2", (p + ".1",), _linattn(p + ".2"), p + ".1", la)); skips.append(p + ".2")
        out.append(Module(p + ".3", (p + ".2",), _down(i, i == L - 1, masked and i < 2), None, ()))
        prev = p + ".3"
    out.append(Module("mid_block1", (prev,), _resblock("mid_block1"), prev, rb))
    out.append(Module("mid_attn", ("mid_block1",), _midattn, "mid_block1", ()))
    out.append(Module("mid_block2", ("mid_attn",), _resblock("mid_block2"), "mid_attn", rb))
    prev = "mid_block2"
    for i in range(L):
        p = f"ups.{i}"                       # ResnetBlock(dim_out + dim_in -> dim_out): a 1x1 res_conv, no identity residual
        out.append(Module(p + ".0", (prev, skips.pop()), _resblock(p + ".0"), None, rb))
        out.append(Module(p + ".1", (p + ".0", skips.pop()), _resblock(p + ".1"), None, rb))
        out.append(Module(p + ".2", (p + ".1",), _linattn(p + ".2"), p + ".1", la))
        out.append(Module(p + ".3", (p + ".2",), _up(i, i == L - 1, masked and i < 2), None, ()))
        prev = p + ".3"
    out.append(Module("final_res_block", (prev, "init"), _resblock("final_res_block"), None, rb))
    out.append(Module("out", ("final_res_block",), _final, None, ()))
    return out


def local_references(sd64: Dict[str, torch.Tensor], temb: torch.Tensor, got: Dict[str, torch.Tensor], mask: Optional[torch.Tensor] = None,
                     internal: bool = False) -> Dict[str, torch.Tensor]:
    """fp64 reference of every module's output (and, with ``internal``, of the training plan's intermediate taps), each computed from
    the taps in ``got`` -- the GPU's -- that the module reads.  ``got`` holds "x" (the network input) and every module's output."""
    groups = fo.unet_meta(sd64)["groups"]
    ctx = Ctx(sd64, temb.double(), None if mask is None else mask.double(), groups)
    refs: Dict[str, torch.Tensor] = {}
    for mod in modules(sd64, masked=mask is not None):
        x = torch.cat([got[n].double().cpu() for n in mod.inputs], dim=1)
        side: Dict[str, torch.Tensor] = {}
        refs[mod.name] = mod.fn(ctx, x, side)
        if internal:
            refs.update({k: v for k, v in side.items() if k.endswith(INTERNAL)})
    return refs


class Row(NamedTuple):
    tap: str
    sample: int
    module: float                   # ||got - ref|| / ||ref||
    branch: float                   # ||got - ref|| / ||ref - x||  (nan: no identity residual)
    ok: bool


def gate(sd64: Dict[str, torch.Tensor], got: Dict[str, torch.Tensor], refs: Dict[str, torch.Tensor], masked: bool = False,
         module_tol: float = MODULE_TOL, branch_tol: float = BRANCH_TOL) -> List[Row]:
    """Per-sample rows for every tap present in both ``got`` and ``refs``."""
    residual = {m.name: m.residual for m in modules(sd64, masked)}
    rows: List[Row] = []
    for name, ref in refs.items():
        if name not in got:
            continue
        g = got[name].double().cpu()
        assert g.shape == ref.shape, (name, tuple(g.shape), tuple(ref.shape))
        d = (g - ref).flatten(1).norm(dim=1)
        rn = ref.flatten(1).norm(dim=1).clamp_min(1e-30)
        res = residual.get(name)
        if res is not None:
            br = (ref - got[res].double().cpu()).flatten(1).norm(dim=1).clamp_min(1e-30)
            bound = branch_tol * br + STORE_FLOOR * g.flatten(1).norm(dim=1)
        for b in range(ref.shape[0]):
            ok = bool(d[b] <= module_tol * rn[b])
            be = float("nan")
            if res is not None:
                be = float(d[b] / br[b])
                ok = ok and bool(d[b] <= bound[b])
            rows.append(Row(name, b, float(d[b] / rn[b]), be, ok))
    return rows


def report(rows: List[Row]) -> str:
    """Worst module error and worst branch error (tap, sample), and every failing row."""
    wm = max(rows, key=lambda r: r.module)
    br = [r for r in rows if r.branch == r.branch]
    s = f"worst module {wm.module:.2e} ({wm.tap}[{wm.sample}])"
    if br:
        wb = max(br, key=lambda r: r.branch)
        s += f", worst branch {wb.branch:.2e} ({wb.tap}[{wb.sample}])"
    bad = [r for r in rows if not r.ok]
    if bad:
        s += f"; {len(bad)} failing rows:\n" + "\n".join(f"  {r.tap:24s} sample {r.sample:3d}  module {r.module:.3e}  branch {r.branch:.3e}"
                                                          for r in bad[:40])
    return s


def worst_sample(got, ref) -> float:
    """The largest per-sample rel-L2 over the leading (batch) dimension: an error in one sample is not diluted by its batch mates."""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    d = (got - ref).flatten(1).norm(dim=1)
    return float((d / ref.flatten(1).norm(dim=1).clamp_min(1e-30)).max())
