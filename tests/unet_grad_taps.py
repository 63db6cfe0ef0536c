"""Module-local fp64 references for the U-Net BACKWARD, and the per-sample gates on them (test helper, imported by
tests/test_gpu_unet_backward_parity.py and tests/test_unet_backward_parity_cpu.py; not a conftest).

The backward plan keeps the gradient of every tapped module output (``fc_unet_debug_tensor("grad:<tap>")``).  ``local_vjp`` rebuilds
each of them from the GPU's OWN forward taps ``x_m`` and the GPU's OWN output cotangents ``dY_m`` (``grad:<module>``; the caller's
``d_out`` for ``out``) with one fp64 surrogate loss, backpropagated once:

    L = sum_m <fn_m(x_m), dY_m>          fn_m: tests/unet_taps.py's module functions (the oracle's), x_m a fresh leaf per (module, input)

so a module's input gradient depends on nothing but that module's arithmetic, and an error stays with the module (and the sample) that
made it.  The state dict, the conditioning vector ``temb`` and the mask are leaves shared by all modules; ``d temb`` is then carried in
fp64 through ``fo.time_embedding`` for the time / class MLPs.  References come out for

    grad:<tap>     the sum of the input gradients of the tap's consumers (skip pops, split concat sources, final_res_block <- init,
                   identity residuals); "dx" / "dmask" the network-input and mask gradients
    parameters     every parameter of the network (None: the parameter takes no part in this step; the GPU must leave it exactly zero)

Gates (per sample b for activations, per tensor for parameters):

    activation     ||got - ref||_b <= G_TOL ||ref||_b
    pass-through   ||got - ref||_b <= BRANCH_TOL ||ref - dY_res||_b + STORE_FLOOR ||got||_b      taps read by an identity residual, whose
                   gradient holds the residual's dY unchanged (the same branch form as unet_taps.gate)
    parameter      ||got - ref|| <= P_TOL ||ref|| + FLOOR_C 2^-24 ||ref_abs||

``ref_abs`` is the rounding scale of the sums the kernels form: each weight-carrying op of the surrogate (conv2d, linear, group_norm,
embedding) adds ``|x| (x) |dy|`` of its own input and output gradient into its parameters' entry (conv: the weight-gradient VJP on |x|
and |dy|, bias: sum |dy|; GroupNorm: sum |dy * xhat|, sum |dy|).  A bias in front of a GroupNorm, whose exact gradient is mostly
cancellation, is then judged against the size of the terms it cancels and not against its own tiny norm.

The branch row reports ``(||got - ref||_b - STORE_FLOOR ||got||_b)+ / ||ref - dY_res||_b``, the part of the error BRANCH_TOL answers for.
The time / class MLPs read the time sinusoid, which the GPU (like the reference) forms in fp32: their reference starts from that fp32
sinusoid, upcast (at time ~ 1e3 its argument carries ~6e-5 rad of rounding, an error of the forward's input and not of the backward).

The bounds are set from the MI355X over the 10 cases of tests/test_gpu_unet_backward_parity.py (~1,650 (tap, sample) rows and ~3,000
parameter tensors): worst activation error 4.4e-7 (dx[1], d8mask), worst branch error beyond the storage floor 9.6e-8 (grad:init[0],
d8mask), worst parameter error 1.9e-6 relative (ups.3.0.block1.proj.bias at 64x64, 0.3 rounding units) and 16.2 rounding units
(ups.0.0.mlp.1.weight at 64x64, 9.7e-7 relative).  G_TOL = 2e-6, BRANCH_TOL = 4e-7, P_TOL = 4e-6 and FLOOR_C = 32 leave a factor of 2-5.
No module needed more than the 1e-5 first proposed: the one that did at first, time_mlp.1.weight at 8e-6, was the fp32 sinusoid above.
"""
from __future__ import annotations

from contextlib import contextmanager
from typing import Dict, List, NamedTuple, Optional

import torch
import torch.nn.functional as F

import unet_taps as ut
from oracle import flow_oracle as fo

G_TOL = 2e-6
BRANCH_TOL = 4e-7
P_TOL = 4e-6
FLOOR_C = 32.0
STORE_FLOOR = ut.STORE_FLOOR
U24 = 2.0 ** -24


class _Recorder:
    """Stands in for ``torch.nn.functional`` inside the oracle while a surrogate is built: every op that reads a parameter is recorded
    with its input and (gradient-retaining) output, so that the absolute-value sums of its parameter gradients can be formed afterwards."""

    def __init__(self, names):
        self.names, self.ops = names, []

    def __getattr__(self, k):
        return getattr(F, k)

    def _rec(self, kind, y, x, w, b, **kw):
        if y.requires_grad and (id(w) in self.names or (b is not None and id(b) in self.names)):
            y.retain_grad()
            self.ops.append((kind, y, x.detach(), w, b, kw))
        return y

    def conv2d(self, x, w, b=None, stride=1, padding=0):
        return self._rec("conv", F.conv2d(x, w, b, stride=stride, padding=padding), x, w, b, stride=stride, padding=padding)

    def linear(self, x, w, b=None):
        return self._rec("linear", F.linear(x, w, b), x, w, b)

    def group_norm(self, x, groups, w=None, b=None, eps=1e-5):
        return self._rec("gn", F.group_norm(x, groups, w, b, eps=eps), x, w, b, groups=groups, eps=eps)

    def embedding(self, idx, w):
        return self._rec("emb", F.embedding(idx, w), idx, w, None)

    def absolute_sums(self) -> Dict[str, torch.Tensor]:
        out: Dict[str, torch.Tensor] = {}

        def add(t, v):
            if t is not None and id(t) in self.names:
                n = self.names[id(t)]
                out[n] = out[n] + v if n in out else v

        for kind, y, x, w, b, kw in self.ops:
            if y.grad is None:
                continue
            gy = y.grad.abs()
            ax = x.abs() if kind != "emb" else x
            if kind == "conv":
                add(w, torch.nn.grad.conv2d_weight(ax, w.shape, gy, stride=kw["stride"], padding=kw["padding"]))
                add(b, gy.sum((0, 2, 3)))
            elif kind == "linear":
                add(w, gy.reshape(-1, gy.shape[-1]).t() @ ax.reshape(-1, ax.shape[-1]))
                add(b, gy.reshape(-1, gy.shape[-1]).sum(0))
            elif kind == "gn":
                xhat = F.group_norm(x, kw["groups"], eps=kw["eps"]).abs()
                add(w, (gy * xhat).sum((0, 2, 3)))
                add(b, gy.sum((0, 2, 3)))
            else:
                add(w, torch.zeros_like(w).index_add_(0, ax.reshape(-1), gy.reshape(-1, w.shape[1])))
        return out


def _sinusoid_fp32(time, dim):
    """The sinusoid the GPU reads (unet.py:18-30 in fp32: the library takes torch's fp32 frequency table and forms time * freq in fp32),
    upcast: at time ~ 1e3 its argument carries ~6e-5 rad of fp32 rounding, an input error of the forward and not of the backward."""
    return _SINUSOID(time.float(), dim).double()


_SINUSOID = fo.sinusoidal_embedding


@contextmanager
def _recording(names, fp32_sinusoid):
    rec = _Recorder(names)
    saved = fo.F, fo.sinusoidal_embedding
    fo.F, fo.sinusoidal_embedding = rec, (_sinusoid_fp32 if fp32_sinusoid else _SINUSOID)
    try:
        yield rec
    finally:
        fo.F, fo.sinusoidal_embedding = saved


class Refs(NamedTuple):
    act: Dict[str, torch.Tensor]            # "grad:<tap>", "dx", "dmask" (fp64)
    passthrough: Dict[str, torch.Tensor]    # "grad:<tap>" -> the dY that identity residuals add to it unchanged
    params: Dict[str, Optional[torch.Tensor]]
    params_abs: Dict[str, torch.Tensor]


def cotangents(sd, got: Dict[str, torch.Tensor], d_out: torch.Tensor, masked: bool = False) -> Dict[str, torch.Tensor]:
    """dY of every module: the GPU's ``grad:<name>`` (in ``got``) and the caller's d_out for the network output."""
    cot = {}
    for m in ut.modules(sd, masked):
        cot[m.name] = (d_out if m.name == "out" else got["grad:" + m.name]).double().cpu()
    return cot


def local_vjp(sd64: Dict[str, torch.Tensor], temb: torch.Tensor, got: Dict[str, torch.Tensor], cot: Dict[str, torch.Tensor],
              time: torch.Tensor, class_cond: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
              fp32_sinusoid: bool = True) -> Refs:
    """References for every activation gradient, d(x), d(mask) and every parameter gradient, from the forward taps in ``got`` ("x" and
    every module output) and the module output cotangents ``cot`` (``cotangents``).  ``temb`` is the conditioning vector the forward
    used (fp64); ``time`` / ``class_cond`` feed the fp64 backward through the time / class MLPs, whose input is the time sinusoid as the
    GPU forms it in fp32 (``fp32_sinusoid``; False: in the dtype of ``time``, for an fp64 oracle)."""
    sd = {k: v.detach().double().cpu().clone().requires_grad_(True) for k, v in sd64.items()}
    names = {id(v): k for k, v in sd.items()}
    te = temb.detach().double().cpu().clone().requires_grad_(True)
    mk = None if mask is None else mask.detach().double().cpu().clone().requires_grad_(True)
    ctx = ut.Ctx(sd, te, mk, fo.unet_meta(sd)["groups"])
    mods = ut.modules(sd64, masked=mask is not None)
    leaves: Dict[str, List[torch.Tensor]] = {}
    passthrough: Dict[str, torch.Tensor] = {}
    with _recording(names, fp32_sinusoid) as rec:
        loss = 0.0
        for m in mods:
            xs = [got[n].detach().double().cpu().clone().requires_grad_(True) for n in m.inputs]
            for n, leaf in zip(m.inputs, xs):
                leaves.setdefault(n, []).append(leaf)
            y = m.fn(ctx, torch.cat(xs, dim=1) if len(xs) > 1 else xs[0], {})
            loss = loss + (y * cot[m.name]).sum()
            if m.residual is not None:
                k = "grad:" + m.residual
                passthrough[k] = passthrough.get(k, 0) + cot[m.name]
        loss.backward()
        # conditioning: d(temb), summed over every ResnetBlock's FiLM, through time_mlp / class_cond_mlp
        t_emb = fo.time_embedding(sd, time.detach().double().cpu(), None if class_cond is None else class_cond.cpu())
        (t_emb * te.grad).sum().backward()
        params_abs = rec.absolute_sums()
    act = {("dx" if n == "x" else "grad:" + n): sum(l.grad for l in ls) for n, ls in leaves.items()}
    if mk is not None:
        act["dmask"] = mk.grad
    params = {k: (None if v.grad is None else v.grad.detach()) for k, v in sd.items()}
    return Refs(act, passthrough, params, params_abs)


class GRow(NamedTuple):
    tap: str
    sample: int
    rel: float                      # ||got - ref||_b / ||ref||_b
    branch: float                   # (||got - ref||_b - STORE_FLOOR ||got||_b)+ / ||ref - dY_res||_b: what BRANCH_TOL bounds (nan: none)
    ok: bool


class PRow(NamedTuple):
    name: str
    rel: float                      # ||got - ref|| / ||ref||  (inf: ref is zero)
    scale: float                    # ||got - ref|| / (2^-24 ||ref_abs||)
    ok: bool


def gate_activations(got: Dict[str, torch.Tensor], refs: Refs, g_tol: float = G_TOL, branch_tol: float = BRANCH_TOL) -> List[GRow]:
    """Per-sample rows for every activation gradient present in both ``got`` and ``refs.act``."""
    rows: List[GRow] = []
    for name, ref in refs.act.items():
        if name not in got:
            continue
        g = got[name].double().cpu()
        assert g.shape == ref.shape, (name, tuple(g.shape), tuple(ref.shape))
        d = (g - ref).flatten(1).norm(dim=1)
        rn = ref.flatten(1).norm(dim=1).clamp_min(1e-300)
        pt = refs.passthrough.get(name)
        if pt is not None:
            br = (ref - pt).flatten(1).norm(dim=1).clamp_min(1e-300)
            store = STORE_FLOOR * g.flatten(1).norm(dim=1)
        for b in range(ref.shape[0]):
            ok = bool(d[b] <= g_tol * rn[b])
            be = float("nan")
            if pt is not None:
                be = float((d[b] - store[b]).clamp_min(0) / br[b])
                ok = ok and be <= branch_tol
            rows.append(GRow(name, b, float(d[b] / rn[b]), be, ok))
    return rows


def gate_params(got: Dict[str, torch.Tensor], refs: Refs, p_tol: float = P_TOL, floor_c: float = FLOOR_C) -> List[PRow]:
    """One row per parameter tensor.  A parameter without a reference gradient (not used this step) must be exactly zero."""
    rows: List[PRow] = []
    for name, ref in refs.params.items():
        g = got[name].double().cpu()
        if ref is None:
            rows.append(PRow(name, 0.0 if not g.any() else float("inf"), 0.0, not bool(g.any())))
            continue
        assert g.shape == ref.shape, (name, tuple(g.shape), tuple(ref.shape))
        d = float((g - ref).norm())
        rn = float(ref.norm())
        ra = float(refs.params_abs[name].norm()) * U24
        ok = d <= p_tol * rn + floor_c * ra
        rows.append(PRow(name, d / rn if rn > 0 else float("inf"), d / ra if ra > 0 else float("inf"), ok))
    return rows


def report(grows: List[GRow], prows: List[PRow]) -> str:
    """Worst activation / branch / parameter errors with their (tap, sample) or tensor, and every failing row."""
    parts = []
    if grows:
        w = max(grows, key=lambda r: r.rel)
        parts.append(f"worst activation {w.rel:.2e} ({w.tap}[{w.sample}])")
        br = [r for r in grows if r.branch == r.branch]
        if br:
            wb = max(br, key=lambda r: r.branch)
            parts.append(f"worst branch {wb.branch:.2e} ({wb.tap}[{wb.sample}])")
    if prows:
        fin = [r for r in prows if r.rel != float("inf") and r.scale != 0.0]
        if fin:
            wp = max(fin, key=lambda r: r.rel)
            ws = max(fin, key=lambda r: r.scale)
            parts.append(f"worst parameter {wp.rel:.2e} ({wp.name}), worst in rounding units {ws.scale:.1f} ({ws.name})")
    s = ", ".join(parts)
    bad_g = [r for r in grows if not r.ok]
    bad_p = [r for r in prows if not r.ok]
    if bad_g or bad_p:
        s += f"; {len(bad_g) + len(bad_p)} failing rows:\n"
        s += "\n".join(f"  {r.tap:28s} sample {r.sample:3d}  rel {r.rel:.3e}  branch {r.branch:.3e}" for r in bad_g[:40])
        if bad_g and bad_p:
            s += "\n"
        s += "\n".join(f"  {r.name:44s} rel {r.rel:.3e}  rounding units {r.scale:.1f}" for r in bad_p[:40])
    return s
