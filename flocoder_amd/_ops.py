"""Thin wrappers over the library's debug hooks, for kernel-level parity tests (not part of the drop-in surface)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _binding as B


def _nhwc(t: Optional[torch.Tensor]):
    return None if t is None else t.permute(0, 2, 3, 1).contiguous()


def conv_debug(x0: torch.Tensor, w: torch.Tensor, bias=None, x1=None, add=None, *, pad=0, stride=1, upsample=False,
               out_act=False, groups_out=0, tile="auto", repeats=0, precision="fp32"):
    """One implicit-GEMM launch.  NCHW in / NCHW out (converted with torch, test plumbing only).
    Returns (out, stats) with stats = (mean, var) per (b, group) reconstructed from the kernel's partials, or None;
    with repeats > 0 returns the average milliseconds of that many back-to-back launches instead."""
    dev = x0.device
    bsz, c0, hs, ws = x0.shape
    cout, cin, ks, _ = w.shape
    c1 = 0 if x1 is None else x1.shape[1]
    assert cin == c0 + c1
    ho = hs * 2 if upsample else (hs + 2 * pad - ks) // stride + 1
    wo = ws * 2 if upsample else (ws + 2 * pad - ks) // stride + 1
    x0n, x1n, addn = _nhwc(x0.float()), _nhwc(None if x1 is None else x1.float()), _nhwc(None if add is None else add.float())
    out = torch.empty(bsz, ho, wo, cout, device=dev, dtype=torch.float32)
    stats = torch.full((bsz * max(groups_out, 1) * 4096 * 2,), float("nan"), device=dev) if groups_out else None
    T, nt, ms = C.c_int(0), C.c_float(0), C.c_float(0)
    tile_id = B.TILE_AUTO if tile == "auto" else B.TILES[tile]
    wc = w.float().contiguous()
    bc = None if bias is None else bias.float().contiguous()
    B.check(B.lib().fc_debug_set_conv_precision(1 if precision == "bf16x3" else 0))
    try:
        B.check(B.lib().fc_debug_conv(B.ptr(x0n), c0, B.ptr(x1n), c1, B.ptr(wc), B.ptr(bc), B.ptr(addn), B.ptr(out), B.ptr(stats),
                                      groups_out, C.byref(T), C.byref(nt), bsz, hs, ws, cout, ks, pad, stride, int(upsample),
                                      int(out_act), tile_id, int(repeats), C.byref(ms), B.current_stream(dev)))
    finally:
        B.check(B.lib().fc_debug_set_conv_precision(0))
    if repeats:
        return ms.value
    res = out.permute(0, 3, 1, 2).contiguous()
    if not groups_out:
        return res, None
    part = stats[: bsz * groups_out * T.value * 2].view(bsz, groups_out, T.value, 2).double()
    mean = part[..., 0].mean(-1)
    m2 = part[..., 1].sum(-1) + nt.value * ((part[..., 0] - mean[..., None]) ** 2).sum(-1)
    var = m2 / (nt.value * T.value)
    return res, (mean, var)


def fetch_tap(model, name: str, batch: int, decode: Optional[bool] = None) -> torch.Tensor:
    """Copy an internal NHWC activation of the model's last forward into a fresh NCHW tensor.  ``decode``: for a codec (``debug_taps``
    on), which of its two plans holds the tap."""
    p, c, h, w = model.debug_tensor(name) if decode is None else model.debug_tensor(name, decode)
    dev = next(model.parameters()).device
    t = torch.empty(batch, h, w, c, device=dev, dtype=torch.float32)
    B.check(B.lib().fc_debug_copy(t.data_ptr(), p, t.numel() * 4, B.current_stream(dev)))
    torch.cuda.synchronize(dev)
    return t.permute(0, 3, 1, 2).contiguous()


def fetch_tap_rows(model, name: str, batch: int, rows: torch.Tensor, rest_any: bool = False):
    """``fetch_tap`` for a large batch: the tap is copied to a device tensor, the samples ``rows`` (an int64 device tensor) are gathered
    there and only they are returned (NCHW, on the device).  With ``rest_any`` also whether any OTHER sample holds a non-zero element
    (``Tensor.any`` on the device): (rows' tensor, bool)."""
    p, c, h, w = model.debug_tensor(name)
    dev = rows.device
    t = torch.empty(batch, h, w, c, device=dev, dtype=torch.float32)
    B.check(B.lib().fc_debug_copy(t.data_ptr(), p, t.numel() * 4, B.current_stream(dev)))
    torch.cuda.synchronize(dev)
    sel = t[rows].permute(0, 3, 1, 2).contiguous()
    if not rest_any:
        return sel
    keep = torch.ones(batch, dtype=torch.bool, device=dev)
    keep[rows] = False
    return sel, bool(t[keep].any())


def ot_pairing(source: torch.Tensor, target: torch.Tensor):
    """Greedy OT pairing on the GPU; returns (perm int64 [B], dist [B,B])."""
    bsz = source.shape[0]
    s = source.reshape(bsz, -1).float().contiguous()
    t = target.reshape(bsz, -1).float().contiguous()
    dist = torch.empty(bsz, bsz, device=s.device, dtype=torch.float32)
    perm = torch.empty(bsz, device=s.device, dtype=torch.int64)
    B.check(B.lib().fc_ot_pairing(B.ptr(s), B.ptr(t), bsz, s.shape[1], B.ptr(dist), B.ptr(perm), B.current_stream(s.device)))
    return perm, dist


def ot_pairing_exact(source: torch.Tensor, target: torch.Tensor, want_duals: bool = True):
    """Exact OT pairing on the GPU; returns (perm int64 [B], cost [B,B] squared distances, duals fp64 [2,B] = (u, v), or None when
    ``want_duals`` is off)."""
    bsz = source.shape[0]
    s = source.reshape(bsz, -1).float().contiguous()
    t = target.reshape(bsz, -1).float().contiguous()
    cost = torch.empty(bsz, bsz, device=s.device, dtype=torch.float32)
    perm = torch.empty(bsz, device=s.device, dtype=torch.int64)
    duals = torch.empty(2, bsz, device=s.device, dtype=torch.float64) if want_duals else None
    B.check(B.lib().fc_ot_pairing_exact(B.ptr(s), B.ptr(t), bsz, s.shape[1], B.ptr(cost), B.ptr(perm), B.ptr(duals), B.current_stream(s.device)))
    return perm, cost, duals


def ot_assign(cost: torch.Tensor):
    """The linear assignment solver alone on a [B,B] cost matrix; returns (perm int64 [B], duals fp64 [2,B] = (u, v))."""
    bsz = cost.shape[0]
    c = cost.reshape(bsz, bsz).float().contiguous()
    perm = torch.empty(bsz, device=c.device, dtype=torch.int64)
    duals = torch.empty(2, bsz, device=c.device, dtype=torch.float64)
    B.check(B.lib().fc_ot_assign(B.ptr(c), bsz, B.ptr(perm), B.ptr(duals), B.current_stream(c.device)))
    return perm, duals


def _sinkhorn_outputs(bsz: int, dev):
    return (torch.empty(bsz, bsz, device=dev, dtype=torch.float32), torch.empty(2, bsz, device=dev, dtype=torch.float64),
            torch.empty(3, device=dev, dtype=torch.float64))


def ot_sinkhorn(cost: torch.Tensor, reg: float, max_iter: int = 1000, stop_thr: float = 1e-9):
    """The log-domain Sinkhorn solver alone on a [B,B] cost matrix; returns (plan fp32 [B,B], duals fp64 [2,B] = (f, g), info fp64 [3]
    = (iterations, converged, err))."""
    bsz = cost.shape[0]
    c = cost.reshape(bsz, bsz).float().contiguous()
    plan, duals, info = _sinkhorn_outputs(bsz, c.device)
    B.check(B.lib().fc_ot_sinkhorn(B.ptr(c), bsz, float(reg), int(max_iter), float(stop_thr), B.ptr(plan), B.ptr(duals), B.ptr(info),
                                   B.current_stream(c.device)))
    return plan, duals, info


def ot_plan_sinkhorn(source: torch.Tensor, target: torch.Tensor, reg: float, normalize_cost: bool = False, max_iter: int = 1000,
                     stop_thr: float = 1e-9):
    """Squared-distance matrix (optionally divided by its maximum) and the Sinkhorn solver; returns (plan, cost [B,B] as the solver saw
    it, duals [2,B], info [3])."""
    bsz = source.shape[0]
    s = source.reshape(bsz, -1).float().contiguous()
    t = target.reshape(bsz, -1).float().contiguous()
    cost = torch.empty(bsz, bsz, device=s.device, dtype=torch.float32)
    plan, duals, info = _sinkhorn_outputs(bsz, s.device)
    B.check(B.lib().fc_ot_plan_sinkhorn(B.ptr(s), B.ptr(t), bsz, s.shape[1], float(reg), int(bool(normalize_cost)), int(max_iter),
                                        float(stop_thr), B.ptr(plan), B.ptr(duals), B.ptr(info), B.ptr(cost), B.current_stream(s.device)))
    return plan, cost, duals, info


def ot_sample_plan(plan: torch.Tensor, n_pairs: int, seed: int = 0, draw_index: int = 0, info: Optional[torch.Tensor] = None):
    """``n_pairs`` index pairs drawn with replacement from a [B,B] plan; returns (i, j) int64 [n_pairs].  ``info``: an int32 [1] device
    tensor that is set to 1 when the plan's sum is not positive and finite."""
    bsz = plan.shape[0]
    p = plan.reshape(bsz, bsz).float().contiguous()
    i = torch.empty(int(n_pairs), device=p.device, dtype=torch.int64)
    j = torch.empty(int(n_pairs), device=p.device, dtype=torch.int64)
    B.check(B.lib().fc_ot_sample_plan(B.ptr(p), bsz, int(n_pairs), int(seed) & 0xffffffffffffffff, int(draw_index), B.ptr(i), B.ptr(j),
                                      B.ptr(info), B.current_stream(p.device)))
    return i, j


def ot_plan_pairing(plan: torch.Tensor):
    """A [B,B] plan as a permutation: row by row the largest entry among the unused columns."""
    bsz = plan.shape[0]
    p = plan.reshape(bsz, bsz).float().contiguous()
    perm = torch.empty(bsz, device=p.device, dtype=torch.int64)
    B.check(B.lib().fc_ot_plan_pairing(B.ptr(p), bsz, B.ptr(perm), B.current_stream(p.device)))
    return perm


def conv_wgrad_debug(x0: torch.Tensor, dy: torch.Tensor, ks: int, x1=None, *, pad=0, stride=1, upsample=False, split_target=0, into=None,
                     geometry=False):
    """Weight / bias gradient of one convolution from its NCHW input(s) and NCHW output gradient: (dW [O,I,KH,KW], db [O]).
    ``split_target``: workgroups wanted per launch (0: the stand-alone default; the backward plan's table entries get 256).  ``into``:
    a (dW, db) pair the gradient is added to (copies of it; the accumulating instantiations).  ``geometry``: also return
    {"nsplit", "mtiles", "TB"} as the launch computed them."""
    dev = x0.device
    bsz, c0, hs, ws = x0.shape
    c1 = 0 if x1 is None else x1.shape[1]
    cout = dy.shape[1]
    x0n, x1n, dyn = _nhwc(x0.float()), _nhwc(None if x1 is None else x1.float()), _nhwc(dy.float())
    if into is None:
        dw = torch.full((cout, c0 + c1, ks, ks), float("nan"), device=dev, dtype=torch.float32)
        db = torch.full((cout,), float("nan"), device=dev, dtype=torch.float32)
    else:
        dw, db = (t.to(dev, torch.float32).clone().contiguous() for t in into)
        assert dw.shape == (cout, c0 + c1, ks, ks) and db.shape == (cout,)
    if not split_target and into is None and not geometry:
        B.check(B.lib().fc_debug_conv_wgrad(B.ptr(x0n), c0, B.ptr(x1n), c1, B.ptr(dyn), cout, bsz, hs, ws, ks, pad, stride, int(upsample),
                                            B.ptr(dw), B.ptr(db), B.current_stream(dev)))
        return dw, db
    ns, mt, tb = C.c_int(0), C.c_int(0), C.c_int(0)
    B.check(B.lib().fc_debug_conv_wgrad_ex(B.ptr(x0n), c0, B.ptr(x1n), c1, B.ptr(dyn), cout, bsz, hs, ws, ks, pad, stride, int(upsample),
                                           B.ptr(dw), B.ptr(db), int(split_target), int(into is not None), C.byref(ns), C.byref(mt),
                                           C.byref(tb), B.current_stream(dev)))
    if not geometry:
        return dw, db
    return dw, db, {"nsplit": ns.value, "mtiles": mt.value, "TB": tb.value}
