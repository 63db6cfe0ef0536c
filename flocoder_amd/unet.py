"""Velocity U-Net: host-side mirror of ``flocoder.unet.Unet`` (reference unet.py:164-377) over the gfx950 library.

Same constructor, same ``forward(x, time, cond)`` protocol, same ``state_dict`` key names and shapes (so the
reference's checkpoints load with ``load_state_dict``), same default initialisation *and RNG consumption order*
(``torch.manual_seed(s); Unet(...)`` gives the reference's weights).  The arithmetic happens in
``libflocoder_amd.so``; this class owns the parameters and hands them over.  There is no CPU path: calling it
with CPU tensors raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
from typing import Dict, List, Optional, Tuple

import torch
from torch import nn

from . import _binding as B
from ._native import NativeModule, read_param_table

# construction order of the reference's Unet.__init__ (unet.py:185-286); state_dict order differs (ups before mid)
_CTOR_ORDER = ["init_conv", "time_mlp", "class_cond_mlp", "mask_fusion_conv", "down_mask_fusions", "up_mask_fusions",
               "downs", "mid_block1", "mid_attn", "mid_block2", "ups", "final_res_block", "final_conv"]
_STATE_ORDER = ["init_conv", "time_mlp", "class_cond_mlp", "mask_fusion_conv", "down_mask_fusions", "up_mask_fusions",
                "downs", "ups", "mid_block1", "mid_attn", "mid_block2", "final_res_block", "final_conv"]


def _make_config(dim, dim_mults, channels, groups, n_classes, mask_cond) -> B.fc_unet_config:
    if len(dim_mults) > 8:
        raise ValueError("at most 8 resolution levels")
    cfg = B.fc_unet_config(dim=int(dim), channels=int(channels), n_levels=len(dim_mults), groups=int(groups),
                           n_classes=max(0, int(n_classes)), mask_cond=int(bool(mask_cond)))
    for i, m in enumerate(dim_mults):
        cfg.dim_mults[i] = int(m)
    return cfg


def param_table(cfg: B.fc_unet_config) -> List[Tuple[str, Tuple[int, ...], int]]:
    """(name, shape, offset into the flat padded vector) as the library lays parameters out.  Needs no GPU."""
    return read_param_table("fc_unet", "create", C.byref(cfg))[0]


def validate_t_eval(t_eval, t0: float, t1: float):
    """solve_ivp's checks of ``t_eval`` over ``(t0, t1)``, with its messages: a sequence, array or tensor -> contiguous fp64 numpy
    array.  (Unlike scipy, a NaN counts as outside the span: no step would ever serve it.)"""
    import numpy as np
    if torch.is_tensor(t_eval):
        t_eval = t_eval.detach().cpu().numpy()
    te = np.asarray(t_eval, dtype=np.float64)
    if te.ndim != 1:
        raise ValueError("`t_eval` must be 1-dimensional.")
    te = np.ascontiguousarray(te)
    if not np.all((te >= min(t0, t1)) & (te <= max(t0, t1))):
        raise ValueError("Values in `t_eval` are not within `t_span`.")
    d = np.diff(te)
    if (t1 > t0 and np.any(d <= 0)) or (t1 < t0 and np.any(d >= 0)):
        raise ValueError("Values in `t_eval` are not properly sorted.")
    return te


def validate_tol(rtol, atol):
    """scipy/integrate/_ivp/common.py validate_tol for scalar tolerances (the warning names the caller of the sampler / integrator
    that was given them)."""
    eps100 = 100 * float(torch.finfo(torch.float64).eps)
    if rtol < eps100:
        import warnings
        warnings.warn(f"At least one element of `rtol` is too small. Setting `rtol = np.maximum(rtol, {eps100})`.", stacklevel=3)
        rtol = eps100
    if atol < 0:
        raise ValueError("`atol` must be positive.")
    return rtol, atol


_GPU_ONLY = "flocoder_amd integrators run on MI355X (gfx950) only"


def require_gpu(x: torch.Tensor, no_cpu_path: bool = True) -> None:
    """The integrators' error for a tensor on the CPU, with or without the trailing clause: every entry keeps the wording it had."""
    if not x.is_cuda:
        raise RuntimeError(_GPU_ONLY + ("; there is no CPU path" if no_cpu_path else ""))


def is_ones_mask(mask: Optional[torch.Tensor]) -> bool:
    """unet.py:301: whether a mask (None counts as not) is all ones.  One host sync: once per call."""
    return mask is not None and bool(torch.allclose(mask, torch.ones_like(mask)))
_SDE_METHODS = {"euler_maruyama": B.FC_SDE_EULER_MARUYAMA, "heun": B.FC_SDE_HEUN}


class _UnetFunction(torch.autograd.Function):
    """Autograd bridge: forward and backward both run in the library; parameters receive ``.grad`` as torch expects, and so do
    ``x`` and the mask when they require it (the inpainting step reaches the MaskEncoder through both, train_flow.py:146-147)."""

    @staticmethod
    def forward(ctx, model, x, time, cls, mask, *params):
        ctx.model, ctx.cls = model, cls
        ctx.save_for_backward(x, time, mask if mask is not None else x.new_empty(0))
        ctx.has_mask = mask is not None
        out = model._forward_native(x, time, cls, mask, train=True)
        ctx.serial = model.arena_serial()
        return out

    @staticmethod
    def backward(ctx, d_out):
        x, time, mask = ctx.saved_tensors
        model = ctx.model
        mask = mask if ctx.has_mask else None
        need_dx, need_dm = ctx.needs_input_grad[1], ctx.has_mask and ctx.needs_input_grad[4]
        if model.arena_serial() != ctx.serial:
            # the library keeps ONE activation arena per model and something wrote it since this graph's forward (a second
            # micro-batch, a validation / sampler call, a re-plan): bring this forward's activations back before differentiating
            model._forward_native(x, time, ctx.cls, mask, train=True)
        flat, dx, dm = model.backward_native(x, time, ctx.cls, d_out, mask=mask, want_dx=need_dx, want_dmask=need_dm)
        grads = []
        for name, shape, off in model._table:
            if ctx.cls is None and name.startswith("class_cond_mlp."):
                grads.append(None)                                # unused this step: p.grad stays None, as in the reference
            elif mask is None and (name.startswith("mask_fusion_conv.") or "_mask_fusions." in name):
                grads.append(None)
            else:
                grads.append(flat[off:off + math.prod(shape)].view(shape).clone())
        return (None, dx, None, None, dm, *grads)


class Unet(NativeModule):
    _fc = "fc_unet"

    def __init__(self, dim, dim_mults=(1, 2, 4, 8), channels=3, resnet_block_groups=4, n_classes=10, mask_cond=False,
                 use_checkpoint=False):
        super().__init__()
        self.use_checkpoint = use_checkpoint      # accepted for signature parity; activations are never stored
        self.channels = channels
        self.out_dim = channels
        self.class_condition = n_classes > 0
        self.dim, self.dim_mults = int(dim), tuple(int(m) for m in dim_mults)
        self._cfg = _make_config(dim, self.dim_mults, channels, resnet_block_groups, n_classes, mask_cond)
        self._read_table()

        # registration in state_dict order, initialisation in constructor order (RNG parity with the reference)
        by_top: Dict[str, List[Tuple[str, Tuple[int, ...]]]] = {}
        for name, shape, _ in self._table:
            by_top.setdefault(name.split(".")[0], []).append((name, shape))
        self._register_table([e for top in _STATE_ORDER for e in by_top.get(top, [])])
        with torch.no_grad():
            for top in _CTOR_ORDER:
                for name, shape in by_top.get(top, []):
                    self._init(name, self.get_parameter(name), by_top[top])

        self._shared = None          # None: decide per call (see _device_is_shared); True / False: set_shared_device

    # ------------------------------------------------------------------ parameters
    @staticmethod
    def _init(name: str, p: nn.Parameter, siblings) -> None:
        """nn.Conv2d / nn.Linear / nn.Embedding / nn.GroupNorm defaults, drawn in the reference's order."""
        leaf = name.rsplit(".", 1)[1]
        if p.dim() == 1 and leaf == "weight":
            p.fill_(1.0)                                        # GroupNorm gain
        elif p.dim() == 1:
            wname = name[: -len("bias")] + "weight"
            wshape = next(s for n, s in siblings if n == wname)
            if len(wshape) == 1:
                p.zero_()                                       # GroupNorm bias
            else:
                bound = 1.0 / math.sqrt(math.prod(wshape[1:]))
                p.uniform_(-bound, bound)                       # Conv2d / Linear bias
        elif name == "class_cond_mlp.0.weight":
            p.normal_(0.0, 1.0)                                 # nn.Embedding
        else:
            nn.init.kaiming_uniform_(p, a=math.sqrt(5))         # Conv2d / Linear weight

    # ------------------------------------------------------------------ native object
    def _create_args(self):
        return (C.byref(self._cfg),)

    def _on_create(self, handle):
        half = self.dim // 2    # frequency table exactly as torch computes it (unet.py:26-27)
        fr = torch.exp(torch.arange(half, dtype=torch.float32) * -(math.log(10000) / (half - 1))).contiguous()
        B.check(B.lib().fc_unet_set_time_freqs(handle, fr.numpy().ctypes.data_as(C.POINTER(C.c_float)), half))

    def _on_use(self, handle, device):
        B.check(B.lib().fc_unet_set_shared(handle, int(self._device_is_shared(device))))
        B.check(B.lib().fc_unet_set_grad_buckets(handle, int(getattr(self, "_grad_buckets", False))))

    def arena_serial(self) -> int:
        """Counter of writes to the library's activation arena (fc_unet_arena_serial)."""
        return int(B.lib().fc_unet_arena_serial(self._handle)) if self._handle else 0

    def reserved_rows(self) -> int:
        """Rows of the current launch plan / activation arena (``fc_unet_reserved``; 0 before the first reservation)."""
        if not self._handle:
            return 0
        rows, h, w = C.c_int(0), C.c_int(0), C.c_int(0)
        B.check(B.lib().fc_unet_reserved(self._handle, C.byref(rows), C.byref(h), C.byref(w)))
        return int(rows.value)

    def reserve(self, rows: int, height: int, width: int, device=None) -> None:
        """Build the launch plan / activation arena for up to `rows` U-Net rows (a CFG sampler needs 2x batch)."""
        device = torch.device(device) if device is not None else next(self.parameters()).device
        B.check(B.lib().fc_unet_reserve(self._native(device), rows, height, width))

    @property
    def flops_per_sample(self) -> float:
        return float(B.lib().fc_unet_flops_per_sample(self._handle)) if self._handle else 0.0

    @property
    def chains(self):
        """(1, reserved rows): the plan runs the batch as one chain of rows (fc_unet_chains, kept for compatibility)."""
        rows = C.c_int(0)
        n = B.lib().fc_unet_chains(self._handle, C.byref(rows)) if self._handle else 0
        return n, rows.value

    def replica(self) -> "Unet":
        """A second model object with the same architecture and (copied) weights on the same device: its own native handle, activation
        arena and captured graphs, so that it can run beside this one on another stream (``sampling.sample_many``)."""
        c = self._cfg
        twin = Unet(self.dim, self.dim_mults, channels=self.channels, resnet_block_groups=int(c.groups), n_classes=int(c.n_classes),
                    mask_cond=bool(c.mask_cond), use_checkpoint=self.use_checkpoint)
        twin.load_state_dict(self.state_dict())
        twin.train(self.training)
        twin = twin.to(next(self.parameters()).device)
        if self._handle:          # same reservation -> same tiles -> bit-identical results (the plan is built for the reserved row count)
            rows, h, w = C.c_int(0), C.c_int(0), C.c_int(0)
            B.check(B.lib().fc_unet_reserved(self._handle, C.byref(rows), C.byref(h), C.byref(w)))
            if rows.value > 0:
                twin.reserve(rows.value, h.value, w.value)
        return twin

    # ------------------------------------------------------------------ device sharing (fc_unet_set_shared)
    def set_shared_device(self, shared: Optional[bool]) -> None:
        """Tell the library whether this model's GPU work runs beside other work it is not ordered against (a second replica meant to
        overlap, the collectives of a training job, another process on the same GPU).  ``True`` selects the plan without
        cross-workgroup waits (same results to fp32 rounding, one more launch per Block); ``False`` insists on the exclusive plan;
        ``None`` (default) decides per call: shared when a process group with more than one rank is live or the caller works on a
        non-default stream, exclusive otherwise."""
        self._shared = shared

    def _device_is_shared(self, device) -> bool:
        if self._shared is not None:
            return bool(self._shared)
        import os
        if os.environ.get("FLOCODER_AMD_SHARED_DEVICE") in ("0", "1"):
            return os.environ["FLOCODER_AMD_SHARED_DEVICE"] == "1"
        d = torch.distributed
        if d.is_available() and d.is_initialized() and d.get_world_size() > 1 and self.training:
            return True          # gradient collectives (RCCL kernels) run beside this model's launches
        return torch.cuda.current_stream(device) != torch.cuda.default_stream(device)

    @property
    def meeting_launches(self) -> int:
        """Launches of the current plan whose workgroups wait for each other (0 on a shared device)."""
        return int(B.lib().fc_unet_meeting_launches(self._handle)) if self._handle else 0

    def check_errors(self, synchronize: bool = True) -> None:
        """Raise RuntimeError if a cross-workgroup wait of a fused Block tail ever timed out on this model (its samples are NaN and
        every later call fails too, until the plan is rebuilt).  With ``synchronize`` the current stream is waited for first, so
        the answer covers everything queued so far."""
        if self._handle:
            B.check(B.lib().fc_unet_check(self._handle, B.current_stream(self._handle_device), int(synchronize)))

    def fused_tail_errors(self) -> int:
        """Timed-out waits of the fused Block tails since the plan was built (must be 0; synchronises)."""
        if not self._handle:
            return 0
        n = C.c_int(0)
        B.check(B.lib().fc_unet_fused_tail_errors(self._handle, C.byref(n)))
        return n.value

    @property
    def launches_per_forward(self) -> int:
        return int(B.lib().fc_unet_plan_launches(self._handle)) if self._handle else 0

    # ------------------------------------------------------------------ forward
    @staticmethod
    def _split_cond(cond):
        if cond is None:
            return None, None
        if not isinstance(cond, dict):
            # the reference dies here too (warnings.DeprecationWarning does not exist)
            raise AttributeError("Non-dict cond signals are dead in the reference; use cond={'class_cond': ids}")
        return cond.get("class_cond"), cond.get("mask_cond")

    def check_class_ids(self, cls: Optional[torch.Tensor]) -> None:
        """nn.Embedding raises IndexError for an id outside [0, n_classes) (unet.py:205,313); the kernels would silently treat such a
        row as unconditional, so the host mirror raises like the reference.  One small host sync per call."""
        if cls is None or cls.numel() == 0:
            return
        mm = torch.stack((cls.min(), cls.max()))
        if mm.is_cuda:
            # The reductions are finished before the copy to the host is issued.  Seen once in tools/inflight_diag.py under
            # FLOCODER_AMD_POISON=1 and AMD_DIRECT_DISPATCH=0 (sample_many, two streams): valid ids read back as 0x00ffffffffffffff /
            # 0x778a00000000 -- what fresh allocator memory holds there, i.e. `mm` before its kernels ran.  Under that switch ROCm 7.2
            # lets work submitted from this thread pass launches still queued in its submission thread, and a stream wait on the host
            # is what orders them (csrc/unet_integrate.hip, the wait before a call's first replay).  Without the poison the leftovers
            # are usually small numbers and the check passes unnoticed, having checked nothing.
            torch.cuda.current_stream(mm.device).synchronize()
        lo, hi = (int(v) for v in mm.tolist())
        if lo < 0 or hi >= self._cfg.n_classes:
            raise IndexError(f"class_cond ids must lie in [0, {self._cfg.n_classes}); got min {lo}, max {hi}")

    def forward(self, x: torch.Tensor, time: torch.Tensor, cond=None) -> torch.Tensor:
        if not x.is_cuda:
            raise RuntimeError("flocoder_amd.Unet runs on MI355X (gfx950) only; there is no CPU path "
                               "(the CPU restatement under oracle/ is test infrastructure).")
        dev = x.device
        bsz, ch, h, w = x.shape
        if ch != self.channels:
            raise ValueError(f"expected {self.channels} input channels, got {ch}")
        cls, mask = self._split_cond(cond)
        x = x.contiguous().float()
        time = time.to(device=dev, dtype=torch.float32).contiguous()
        if time.shape != (bsz,):
            raise ValueError("time must have shape [batch]")
        if cls is not None and not self.class_condition:
            cls = None                                            # hasattr(self,'class_cond_mlp') is False, unet.py:315
        if cls is not None:
            cls = cls.to(device=dev, dtype=torch.int64).contiguous()
            if cls.shape != (bsz,):
                raise ValueError("class_cond must have shape [batch]")
            self.check_class_ids(cls)
        if mask is not None and not self._cfg.mask_cond:
            mask = None                                           # hasattr(self,'mask_fusion_conv') is False, unet.py:298
        if mask is not None:
            mask = mask.to(device=dev, dtype=torch.float32).contiguous()
            if mask.shape != x.shape:
                raise ValueError("mask_cond must have the shape of x (unet.py:302)")
        if torch.is_grad_enabled() and self.training and any(p.requires_grad for p in self.parameters()):
            # loss.backward() support (train_flow.py:358-371): gradients come from the library's backward plan
            params = [self.get_parameter(n) for n, _, _ in self._table]
            return _UnetFunction.apply(self, x, time, cls, mask, *params)
        return self._forward_native(x, time, cls, mask, train=False)

    def _forward_native(self, x, time, cls, mask, train: bool) -> torch.Tensor:
        dev = x.device
        bsz, _, h, w = x.shape
        ones = int(is_ones_mask(mask))                            # one host sync, as upstream
        hnd = self._native(dev)
        B.check((B.lib().fc_unet_train_reserve if train else B.lib().fc_unet_reserve)(hnd, bsz, h, w))
        out = torch.empty_like(x)
        B.check(B.lib().fc_unet_forward(hnd, B.ptr(x), B.ptr(time), B.ptr(cls), B.ptr(mask), ones, B.ptr(out), bsz, h, w,
                                        B.current_stream(dev)))
        return out

    def set_grad_buckets(self, on: bool) -> None:
        """Build the backward plan in its two-bucket form (``fc_unet_set_grad_buckets``): data-parallel trainers, so that the all-reduce of
        the late layers' gradients can start in the middle of the backward."""
        self._grad_buckets = bool(on)

    def grad_buckets(self) -> Tuple[int, int]:
        """(number of gradient buckets of the current backward plan, flat offset where the early bucket starts): after part 0 of
        ``backward_native`` the range [offset, numel) -- final_*, mid_*, ups.* -- is final, part 1 completes [0, offset)."""
        off = C.c_int64(0)
        n = B.lib().fc_unet_grad_buckets(self._handle, C.byref(off)) if self._handle else 0
        return int(n), int(off.value)

    def backward_native(self, x, time, cls, d_out, grads: Optional[torch.Tensor] = None, mask=None, want_dx=False, want_dmask=False,
                        parts: Tuple[int, int] = (0, 1), dx=None, dm=None, accumulate: bool = False):
        """Parameter gradients of the LAST training forward (same x / time / class ids / mask) for d(out) = ``d_out``: a flat fp32
        vector in the library's table layout (``grad_views`` splits it), plus d(x) / d(mask) on request.  Returns
        ``(flat, dx | None, dmask | None)``.  train_flow.py:371 loss.backward().  ``parts`` = (first, last) of the two halves of the
        backward plan (``fc_unet_backward_parts``): (0, 0) stops behind mid_block1 with the late-layer gradients final, (1, 1) runs the
        rest -- a data-parallel trainer all-reduces the first bucket in between.  ``accumulate`` (``fc_unet_backward_accumulate``): the
        gradients are ADDED to what ``grads`` holds and every element without a gradient in this call is left untouched; d(x) / d(mask)
        are overwritten as before."""
        dev = x.device
        bsz, _, h, w = x.shape
        if grads is None:
            if accumulate:
                raise ValueError("backward_native(accumulate=True) needs the gradient vector to add to")
            grads = torch.empty(self._flat_numel, dtype=torch.float32, device=dev)
        ones = int(is_ones_mask(mask))
        if dx is None:
            dx = torch.empty_like(x) if want_dx else None
        if dm is None:
            dm = torch.empty_like(x) if (want_dmask and mask is not None) else None
        entry = B.lib().fc_unet_backward_accumulate if accumulate else B.lib().fc_unet_backward_parts
        B.check(entry(self._native(dev), B.ptr(x), B.ptr(time), B.ptr(cls), B.ptr(mask), ones, B.ptr(d_out.contiguous()),
                      B.ptr(grads), grads.numel(), B.ptr(dx), B.ptr(dm), bsz, h, w, int(parts[0]), int(parts[1]), B.current_stream(dev)))
        return grads, dx, dm

    def vjp_x(self, x, time, cls, d_out, mask=None) -> torch.Tensor:
        """d(x) of the LAST training forward (same x / time / class ids / mask) for d(out) = ``d_out``, and nothing else
        (``fc_unet_vjp_x``): the backward plan's data-gradient chain without any launch that only serves parameter gradients.  The bits
        are those of ``backward_native(..., want_dx=True)[1]``; no flat gradient vector is touched."""
        dev = x.device
        bsz, _, h, w = x.shape
        ones = int(is_ones_mask(mask))
        dx = torch.empty_like(x)
        B.check(B.lib().fc_unet_vjp_x(self._native(dev), B.ptr(x), B.ptr(time), B.ptr(cls), B.ptr(mask), ones, B.ptr(d_out.contiguous()),
                                      B.ptr(dx), bsz, h, w, B.current_stream(dev)))
        return dx

    def vjp_forms(self) -> List[Tuple[str, str]]:
        """(kernel family, module) of every backward-plan entry ``vjp_x`` runs (``fc_unet_vjp_op_info``; tests, tools)."""
        out = []
        for i in range(B.lib().fc_unet_vjp_launches(self._handle) if self._handle else 0):
            k, m = C.c_char_p(), C.c_char_p()
            B.check(B.lib().fc_unet_vjp_op_info(self._handle, i, C.byref(k), C.byref(m)))
            out.append((k.value.decode(), m.value.decode()))
        return out

    def grad_views(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        return {name: flat[off:off + math.prod(shape)].view(shape) for name, shape, off in self._table}

    def param_range(self, *prefixes) -> Tuple[int, int]:
        """[lo, hi) inside the flat table of the (contiguous) parameters whose names start with one of ``prefixes``."""
        names = [(off, off + (math.prod(shape) + 3) // 4 * 4) for name, shape, off in self._table if name.startswith(tuple(prefixes))]
        return (min(a for a, _ in names), max(b for _, b in names)) if names else (0, 0)

    def class_param_range(self) -> Tuple[int, int]:
        """class_cond_mlp.*: no gradient when a step runs without conditioning."""
        return self.param_range("class_cond_mlp.")

    def adopt_flat(self, flat: torch.Tensor) -> None:
        """Make every parameter a view into ``flat`` (table layout) so that an optimiser working on the flat vector updates the
        module in place; ``sync_flat`` then hands the new values to the library without a gather."""
        with torch.no_grad():
            for name, shape, off in self._table:
                p = self.get_parameter(name)
                flat[off:off + math.prod(shape)].copy_(p.detach().reshape(-1))
                p.data = flat[off:off + math.prod(shape)].view(shape)
        self._flat = flat

    def sync_flat(self) -> None:
        flat = self._flat
        hnd = self._native(flat.device) if self._handle is None else self._handle
        B.check(B.lib().fc_unet_load_params(hnd, flat.data_ptr(), flat.numel(), 1, B.current_stream(flat.device)))
        self._synced = self._weights_version()

    # ------------------------------------------------------------------ integrators (used by flocoder_amd.sampling)
    def _integrator_args(self, x, class_ids, mask, cfg_strength=0.0):
        """What every integrator method checks of ``x`` and does to its conditioning -> ``(class ids, mask, U-Net rows per evaluation,
        native handle)``: ids as int64 ``[batch]`` in range, or None for a model without classes; the mask as fp32 of x's shape, or None
        for a model without mask conditioning; a guided call evaluates two rows per sample."""
        require_gpu(x)
        dev = x.device
        bsz = x.shape[0]
        if not x.is_contiguous() or x.dtype != torch.float32:
            raise ValueError("x must be a contiguous fp32 tensor (it is updated in place)")
        if class_ids is not None and not self.class_condition:
            class_ids = None
        if class_ids is not None:
            class_ids = class_ids.to(device=dev, dtype=torch.int64).contiguous()
            if class_ids.shape != (bsz,):
                raise ValueError("class ids must have shape [batch]")
            self.check_class_ids(class_ids)
        if mask is not None and not self._cfg.mask_cond:
            mask = None
        if mask is not None:
            mask = mask.to(device=dev, dtype=torch.float32).contiguous()
            if mask.shape != x.shape:
                raise ValueError("mask_cond must have the shape of x")
        rows = bsz * (2 if (class_ids is not None and cfg_strength) else 1)
        return class_ids, mask, rows, self._native(dev)

    @staticmethod
    def _integrator_check(hnd, dev, check: bool) -> None:
        """The tail of every integrator method: with ``check``, wait for the trajectory when the plan contains cross-workgroup waits and
        raise if one timed out."""
        if check and B.lib().fc_unet_meeting_launches(hnd) > 0:
            B.check(B.lib().fc_unet_check(hnd, B.current_stream(dev), 1))

    @staticmethod
    def _host_grid(ts: torch.Tensor, min_points: int = 0):
        """``ts`` as the library reads it -> ``(host fp32 tensor, its ctypes pointer, number of points)``; the tensor owns the memory."""
        ts_host = ts.detach().to("cpu", torch.float32).contiguous()
        if ts_host.numel() < min_points:
            raise ValueError(f"the time grid needs at least {'two' if min_points == 2 else min_points} points")
        return ts_host, ts_host.numpy().ctypes.data_as(C.POINTER(C.c_float)), ts_host.numel()

    @staticmethod
    def _check_aligned(x: torch.Tensor) -> None:
        if x.data_ptr() % 16:
            raise ValueError("x must be 16-byte aligned (the kernels read it as float4)")

    @contextlib.contextmanager
    def _training_form(self, hnd, bsz: int, h: int, w: int, restore: bool):
        """The body runs with the plans in the training form (every intermediate kept, none of the fused inference launches), which
        ``fc_unet_train_reserve`` switches a handle to for good.  With ``restore``, a model that was NOT in that form -- one that trains is
        left as it is -- gets its inference plans and the reservation it had back behind the body."""
        lib = B.lib()
        was_training_form = bool(lib.fc_unet_train_form(hnd))
        rows0, h0, w0 = C.c_int(0), C.c_int(0), C.c_int(0)
        B.check(lib.fc_unet_reserved(hnd, C.byref(rows0), C.byref(h0), C.byref(w0)))
        B.check(lib.fc_unet_train_reserve(hnd, bsz, h, w))
        yield
        if restore and not was_training_form:
            self.release_training_plan()
            if rows0.value > 0:                         # the reservation the caller had, in the form it had
                B.check(lib.fc_unet_reserve(hnd, rows0.value, h0.value, w0.value))

    def integrate(self, method: str, x: torch.Tensor, ts: torch.Tensor, *, dt_euler: float = 0.0, t_scale: float = 999.0,
                  class_ids: Optional[torch.Tensor] = None, cfg_strength: float = 0.0, mask: Optional[torch.Tensor] = None,
                  mask_is_ones: bool = False, check: bool = True) -> torch.Tensor:
        """Integrate ``x`` in place along the fp32 grid ``ts`` with the hipGraph-captured step; returns ``x``.  With ``check`` (default)
        the call waits for the trajectory when the plan contains cross-workgroup waits and raises if one timed out -- a caller never
        receives samples from a plan whose residency assumption broke.  ``check=False`` keeps the call asynchronous; the error then
        surfaces at the next call on the model or at ``check_errors()``."""
        require_gpu(x, no_cpu_path=False)                         # this entry's wording has no trailing clause
        class_ids, mask, rows, hnd = self._integrator_args(x, class_ids, mask, cfg_strength)
        code = {"euler": B.FC_METHOD_EULER, "rk4": B.FC_METHOD_RK4}[method]
        dev = x.device
        bsz, _, h, w = x.shape
        B.check(B.lib().fc_unet_reserve(hnd, rows, h, w))
        _, ts_ptr, n_points = self._host_grid(ts)
        B.check(B.lib().fc_unet_integrate(hnd, code, B.ptr(x), bsz, h, w, ts_ptr, n_points, float(dt_euler), float(t_scale), B.ptr(class_ids),
                                          float(cfg_strength or 0.0), B.ptr(mask), int(mask_is_ones), B.current_stream(dev)))
        self._integrator_check(hnd, dev, check)
        return x

    @staticmethod
    def _probes_arg(x: torch.Tensor, probe: torch.Tensor):
        """A likelihood call's probe argument: x's shape (one probe: today's call) or ``[K, *x.shape]`` (K probes in one solve).  Returns
        (probe, K or None), the probe 16-byte aligned."""
        several = probe.dim() == x.dim() + 1
        if (probe.shape[1:] if several else probe.shape) != x.shape or probe.device != x.device or probe.dtype != torch.float32 \
                or not probe.is_contiguous():
            raise ValueError("probe must be a contiguous fp32 tensor of x's shape, or [K, *x.shape] for K probes, on x's device")
        if several and not 1 <= probe.shape[0] <= B.FC_LL_MAX_PROBES:
            raise ValueError(f"n_probes={probe.shape[0]} must lie in [1, {B.FC_LL_MAX_PROBES}] (the cap on probes per call)")
        if probe.data_ptr() % 16:
            probe = probe.clone()                       # a view at an odd storage offset: the kernels read the probe as float4
        return probe, (int(probe.shape[0]) if several else None)

    def _likelihood_call(self, name: str, hnd, x, probe, k, head, mid=(), tail=(), *, check: bool, restore_plan: bool):
        """Allocate a likelihood call's outputs ``(a, logp)``, for K probes ``(a, logp, a_probes, stderr)``, and run its native entry in the
        training form of the plans: ``name`` for one probe (``k`` None), ``name_probes`` for K, which takes K behind the probe.  ``head``:
        the arguments between x's dimensions and the probe, ``mid``: between the probe and the outputs, ``tail``: behind them."""
        dev = x.device
        bsz, _, h, w = x.shape
        out = tuple(torch.empty(bsz, dtype=torch.float64, device=dev) for _ in range(2))
        if k is not None:
            out += (torch.empty(k, bsz, dtype=torch.float64, device=dev), torch.empty(bsz, dtype=torch.float64, device=dev))
        entry = getattr(B.lib(), name if k is None else name + "_probes")
        with self._training_form(hnd, bsz, h, w, restore_plan):
            B.check(entry(hnd, B.ptr(x), bsz, h, w, *head, B.ptr(probe), *(() if k is None else (k,)), *mid, *(B.ptr(t) for t in out), *tail,
                          B.current_stream(dev)))
            self._integrator_check(hnd, dev, check)
        return out

    @staticmethod
    def _public_counters(counters, bsz: int, per_sample: bool):
        """The native RK45 counters -> ``(nfev, accepted, rejected)``: ints, or per sample int64 CPU tensors ``[B]``."""
        if per_sample:
            c = torch.tensor(list(counters), dtype=torch.int64).view(bsz, 3)
            return (c[:, 0].clone(), c[:, 1].clone(), c[:, 2].clone())
        return (int(counters[0]), int(counters[1]), int(counters[2]))

    def log_likelihood(self, x: torch.Tensor, ts: torch.Tensor, probe: torch.Tensor, *, t_scale: float = 999.0,
                       class_ids: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, mask_is_ones: bool = False,
                       check: bool = True, restore_plan: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
        """``fc_unet_log_likelihood``: integrate ``x`` in place along the fp32 grid ``ts`` (the sampler's grid reversed: data -> noise)
        with the RK4 step, carrying the Hutchinson divergence estimate for ``probe`` (x's shape) next to it.  Returns ``(a, logp)``, fp64
        ``[B]`` on x's device: the integrated divergence and ``-|z|^2/2 - (CHW/2) ln 2pi + a`` with ``z`` = the ``x`` left behind.  Argument
        checks and ``check`` as in ``integrate``; no guidance.

        The loop needs the backward plan, hence the training form of the plans (``_training_form``).  A model that was NOT in that form
        gets its inference form back before the call returns (``restore_plan``, default): later sampler calls run the plan, and give the
        bits, of a model that never computed a likelihood, at the cost of a device synchronisation and two plan builds per call.  For many
        likelihood calls in a row pass ``restore_plan=False`` and call ``release_training_plan()`` once at the end.

        ``probe`` of shape ``[K, *x.shape]`` (``fc_unet_log_likelihood_probes``, 1 <= K <= 64): K probes in one solve -- one forward per
        evaluation and K data-gradient chains behind it.  Returns ``(a, logp, a_probes, logp_stderr)``: ``a_probes`` fp64 ``[K, B]``, row k
        with the bits of a single-probe call with probe k; ``a`` their mean (summed in probe order, one division), ``logp`` formed from
        it; ``logp_stderr`` fp64 ``[B]`` = ``sqrt(sum_k (a_k - a)^2 / (K (K - 1)))``, NaN for K = 1."""
        class_ids, mask, _, hnd = self._integrator_args(x, class_ids, mask)
        probe, k = self._probes_arg(x, probe)
        _, ts_ptr, n_points = self._host_grid(ts, 2)
        return self._likelihood_call("fc_unet_log_likelihood", hnd, x, probe, k,
                                     (ts_ptr, n_points, float(t_scale), B.ptr(class_ids), B.ptr(mask), int(mask_is_ones)),
                                     check=check, restore_plan=restore_plan)

    def log_likelihood_rk45(self, x: torch.Tensor, eps: torch.Tensor, t0: float = 1.0, t1: float = 0.0, rtol: float = 1e-5,
                            atol: float = 1e-5, per_sample: bool = True, *, t_scale: float = 999.0, class_ids: Optional[torch.Tensor] = None,
                            mask: Optional[torch.Tensor] = None, mask_is_ones: bool = False, check: bool = True, restore_plan: bool = True):
        """``fc_unet_log_likelihood_rk45``: ``log_likelihood`` with error control.  ``x`` is integrated in place from ``t0`` back to ``t1``
        (``0 <= t1 < t0 <= 1``) by scipy's adaptive RK45 (``integrate_rk45``'s controller) on the concatenated state ``[x, a]``,
        ``da[b]/dt = sum eps (dv/dx)^T eps`` with the probe ``eps`` (x's shape), ``a = 0`` at ``t0``: the divergence integral takes part
        in the error norm and the step control.  ``per_sample=True`` (default: a sample's likelihood is its own quantity) solves every
        sample as its own problem over its C*H*W + 1 unknowns; ``per_sample=False`` is one problem over the batch, as the literature's
        code.  Returns ``(counters, a, logp)``: ``counters = (nfev, accepted, rejected)`` as ``integrate_rk45`` returns them (ints, or int64
        CPU tensors ``[B]`` per sample); ``a`` and ``logp = -|z|^2/2 - (CHW/2) ln 2pi + a`` fp64 ``[B]`` on x's device, ``z`` = the ``x`` left
        behind.  Synchronous.  A failed solve raises RuntimeError with scipy's message (per sample naming the samples) and leaves ``x``
        untouched.  The form of the plans is handled as in ``log_likelihood`` (``restore_plan``).

        ``eps`` of shape ``[K, *x.shape]`` (``fc_unet_log_likelihood_rk45_probes``): the state stays ``[x, a]`` with ``da/dt`` the MEAN of
        the K probes' estimates (summed in probe order, one division), so K copies of one probe give the single-probe solve bit for bit;
        every evaluation is one forward and K chains.  Returns ``(counters, a, logp, a_probes, logp_stderr)``: ``a_probes`` fp64 ``[K, B]``,
        every probe's own integral over the accepted steps (by-products outside the error norm; their mean equals ``a`` up to fp64
        rounding), ``logp_stderr`` as in ``log_likelihood`` around ``a``."""
        rtol, atol = validate_tol(rtol, atol)
        t0, t1 = float(t0), float(t1)
        if not (0.0 <= t1 < t0 <= 1.0):
            raise ValueError(f"t0={t0}, t1={t1}: the likelihood is integrated from the data end back towards noise, 0 <= t1 < t0 <= 1")
        class_ids, mask, _, hnd = self._integrator_args(x, class_ids, mask)
        bsz = x.shape[0]
        eps, k = self._probes_arg(x, eps)
        self._check_aligned(x)
        counters = (C.c_int * (3 * bsz if per_sample else 3))()
        out = self._likelihood_call("fc_unet_log_likelihood_rk45", hnd, x, eps, k,
                                    (t0, t1, float(rtol), float(atol), float(t_scale), B.ptr(class_ids), B.ptr(mask), int(mask_is_ones)),
                                    mid=(int(per_sample),), tail=(counters,), check=check, restore_plan=restore_plan)
        return (self._public_counters(counters, bsz, per_sample),) + out

    def integrate_guided(self, x: torch.Tensor, ts: torch.Tensor, measurement: torch.Tensor, keep: torch.Tensor, *, sigma_y: float = 0.05,
                         gamma: float = 1.0, jacobian: str = "identity", t_scale: float = 999.0, class_ids: Optional[torch.Tensor] = None,
                         cfg_strength: float = 0.0, mask: Optional[torch.Tensor] = None, mask_is_ones: bool = False, check: bool = True,
                         restore_plan: bool = True) -> torch.Tensor:
        """``fc_unet_integrate_guided``: integrate ``x`` in place along the fp32 grid ``ts`` (every point > 0) with the RK4 step, every stage
        velocity corrected towards ``measurement = keep * x1`` (``inpainting.algorithm3`` for a diagonal operator); returns ``x``.
        ``measurement`` has x's shape, ``keep`` x's shape or ``[B,1,H,W]``.  ``jacobian="identity"`` is the captured path: class ids,
        guidance, mask and ``check`` as ``integrate``.  ``jacobian="exact"`` adds ``(1-t) (dv/dx)^T w`` through the backward plan's
        data-gradient chain; it takes no classifier-free guidance and needs the training form of the plans, which it handles as
        ``log_likelihood`` does: a model that was not in that form gets its inference plans and reservation back before the call returns
        unless ``restore_plan=False`` (then ``release_training_plan()`` is the caller's)."""
        if jacobian not in ("identity", "exact"):
            raise ValueError(f"jacobian={jacobian!r}: 'identity' or 'exact'")
        exact = jacobian == "exact"
        if exact and class_ids is not None and self.class_condition and cfg_strength:
            raise ValueError("jacobian='exact' takes no classifier-free guidance: the chain differentiates one forward, not the guided pair")
        class_ids, mask, rows, hnd = self._integrator_args(x, class_ids, mask, cfg_strength)
        dev = x.device
        bsz, _, h, w = x.shape
        if measurement.shape != x.shape:
            raise ValueError(f"measurement must have the shape of x {tuple(x.shape)}, got {tuple(measurement.shape)}")
        if tuple(keep.shape) not in (tuple(x.shape), (bsz, 1, h, w)):
            raise ValueError(f"keep must have the shape of x or [B,1,H,W], got {tuple(keep.shape)}")
        if sigma_y < 0:
            raise ValueError("sigma_y must be >= 0")
        ts_host, ts_ptr, n_points = self._host_grid(ts, 2)
        self._check_aligned(x)
        # fresh aligned fp32 copies on x's device (the library copies them again into its own buffers)
        ym = measurement.to(device=dev, dtype=torch.float32).contiguous().clone()
        kp = keep.to(device=dev, dtype=torch.float32).expand_as(x).contiguous().clone()
        if not bool((ts_host > 0).all()):
            raise ValueError("every grid point must be > 0: the correction is gamma (1-t)/t g")
        if not exact:
            B.check(B.lib().fc_unet_reserve(hnd, rows, h, w))
        with self._training_form(hnd, bsz, h, w, restore_plan) if exact else contextlib.nullcontext():
            B.check(B.lib().fc_unet_integrate_guided(hnd, B.ptr(x), bsz, h, w, ts_ptr, n_points, float(t_scale), B.ptr(class_ids),
                                                     float(cfg_strength or 0.0), B.ptr(mask), int(mask_is_ones), B.ptr(ym), B.ptr(kp), float(sigma_y),
                                                     float(gamma), B.FC_JACOBIAN_EXACT if exact else B.FC_JACOBIAN_IDENTITY, B.current_stream(dev)))
            self._integrator_check(hnd, dev, check)
        return x

    def integrate_sde(self, x: torch.Tensor, ts: torch.Tensor, *, sigma: float, method: str, seed: int = 0,
                      sample_ids: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                      class_ids: Optional[torch.Tensor] = None, cfg_strength: float = 0.0, mask: Optional[torch.Tensor] = None,
                      mask_is_ones: bool = False, t_scale: float = 999.0, check: bool = True) -> torch.Tensor:
        """``fc_unet_integrate_sde``: integrate ``x`` in place along the fp32 grid ``ts`` (non-decreasing, within [0, 1]) with the SDE that
        shares the flow's marginals, ``dx = ((1 + sigma^2 t/2) v - sigma^2 x/2) dt + sigma sqrt(1-t) dW``; returns ``x``.  ``method``:
        ``"euler_maruyama"`` (one evaluation per interval) or ``"heun"`` (two, one noise draw).  The noise of interval i is ``noise[i]``
        (fp32 ``[len(ts)-1, *x.shape]`` on x's device) or, without ``noise``, the library's counter-based normal field
        (``flocoder_amd.noise``) of ``seed`` and the per-row ``sample_ids`` (int64 ``[B]``, default ``arange(B)``): a row's noise follows its
        id, not its position or the batch size.  Class ids, guidance, mask and ``check`` as ``integrate``."""
        if method not in _SDE_METHODS:
            raise ValueError(f"method={method!r}: one of {sorted(_SDE_METHODS)}")
        sigma = float(sigma)
        if not (sigma >= 0 and math.isfinite(sigma)):
            raise ValueError("sigma must be finite and >= 0")
        class_ids, mask, rows, hnd = self._integrator_args(x, class_ids, mask, cfg_strength)
        dev = x.device
        bsz, _, h, w = x.shape
        self._check_aligned(x)
        ts_host, ts_ptr, n_points = self._host_grid(ts, 2)
        if ts_host.dim() != 1:
            raise ValueError("the time grid needs at least two points")
        if not bool(((ts_host >= 0) & (ts_host <= 1)).all()) or not bool((ts_host[1:] >= ts_host[:-1]).all()):
            raise ValueError("the time grid must be non-decreasing within [0, 1]")
        if noise is not None:
            if tuple(noise.shape) != (ts_host.numel() - 1,) + tuple(x.shape) or noise.device != dev:
                raise ValueError(f"noise must have shape {(ts_host.numel() - 1,) + tuple(x.shape)} on x's device, got {tuple(noise.shape)} "
                                 f"on {noise.device}")
            noise = noise.to(torch.float32).contiguous()
            if noise.data_ptr() % 16:
                noise = noise.clone()
        if sample_ids is None:
            sample_ids = torch.arange(bsz, dtype=torch.int64, device=dev)
        if sample_ids.dtype != torch.int64 or tuple(sample_ids.shape) != (bsz,):
            raise ValueError("sample_ids must be an int64 tensor of shape [batch]")
        sample_ids = sample_ids.to(dev).contiguous()
        lib = B.lib()
        B.check(lib.fc_unet_reserve(hnd, rows, h, w))
        B.check(lib.fc_unet_integrate_sde(hnd, _SDE_METHODS[method], B.ptr(x), bsz, h, w, ts_ptr, n_points, float(t_scale), B.ptr(class_ids),
                                          float(cfg_strength or 0.0), B.ptr(mask), int(mask_is_ones), sigma, int(seed) & 0xffffffffffffffff,
                                          B.ptr(sample_ids), B.ptr(noise), B.current_stream(dev)))
        self._integrator_check(hnd, dev, check)
        return x

    def release_training_plan(self) -> None:
        """Put the handle's plans back into the inference form (``fc_unet_train_release``): waits for the device, drops the training-form
        plans, the backward plan and the captured graphs; the next call builds what a model that never trained builds."""
        if self._handle:
            B.check(B.lib().fc_unet_train_release(self._handle))

    def integrate_rk45(self, x: torch.Tensor, t0: float, t1: float, *, rtol: float, atol: float, t_scale: float = 999.0,
                       class_ids: Optional[torch.Tensor] = None, cfg_strength: float = 0.0, mask: Optional[torch.Tensor] = None,
                       mask_is_ones: bool = False, check: bool = True, per_sample: bool = False, t_eval=None):
        """Integrate ``x`` in place from ``t0`` to ``t1`` with scipy's adaptive RK45 (``fc_unet_integrate_rk45``: solve_ivp semantics,
        one step size and one error norm for the whole batch, so a sample's trajectory depends on the rest of its batch as upstream).
        Synchronous: the host waits for a small status record behind every attempt of six evaluations.  Returns ``(nfev, accepted,
        rejected)``; ``nfev`` is scipy's ``solution.nfev`` (a CFG pair counts once).  Raises RuntimeError when the step size falls below
        the spacing of t (scipy's ``success=False``) and ValueError for ``atol < 0``.

        ``per_sample=True`` (``fc_unet_integrate_rk45_per_sample``) solves every sample as its own solve_ivp problem (own initial step,
        error norm, step size and counters), so a sample's result depends only on its own source, class id and mask.  It then returns
        ``(nfev, accepted, rejected)`` as int64 CPU tensors of shape [B]; the call makes ``nfev.max()`` batch forwards.  A failing
        sample raises RuntimeError naming it, and ``x`` is left untouched.

        ``t_eval`` (a sequence, array or tensor of times; ``fc_unet_integrate_rk45_dense``) is solve_ivp's: the steps, ``x`` and the
        counters are those of the call without it, and the return value gains ``frames``, an fp32 tensor ``[F, B, C, H, W]`` on
        ``x``'s device: frame j is the trajectory at ``t_eval[j]``, evaluated from the quartic interpolant of the accepted step that
        contains it (in per-sample mode each sample's own step).  The times must lie in ``[t0, t1]`` and be strictly monotonic in the
        direction of integration (ValueError with scipy's messages otherwise, before anything else is looked at).  When the solve
        fails the frames are discarded with it."""
        te = None if t_eval is None else validate_t_eval(t_eval, t0, t1)
        rtol, atol = validate_tol(rtol, atol)
        class_ids, mask, rows, hnd = self._integrator_args(x, class_ids, mask, cfg_strength)
        dev = x.device
        bsz, _, h, w = x.shape
        B.check(B.lib().fc_unet_reserve(hnd, rows, h, w))
        counters = (C.c_int * (3 * bsz if per_sample else 3))()
        head = (B.ptr(x), bsz, h, w, float(t0), float(t1), float(rtol), float(atol), float(t_scale), B.ptr(class_ids),
                float(cfg_strength or 0.0), B.ptr(mask), int(mask_is_ones))
        frames = None
        if te is None:
            fn = B.lib().fc_unet_integrate_rk45_per_sample if per_sample else B.lib().fc_unet_integrate_rk45
            B.check(fn(hnd, *head, counters, B.current_stream(dev)))
        else:
            frames = torch.empty((len(te),) + tuple(x.shape), dtype=torch.float32, device=dev)
            B.check(B.lib().fc_unet_integrate_rk45_dense(hnd, int(per_sample), *head, te.ctypes.data_as(C.POINTER(C.c_double)), len(te),
                                                         B.ptr(frames), counters, B.current_stream(dev)))
        self._integrator_check(hnd, dev, check)
        out = self._public_counters(counters, bsz, per_sample)
        return out if te is None else out + (frames,)

    def profile_ops(self, batch: int, repeats: int = 20):
        """Per-launch device time of the current plan (bench.py's live roofline measurement).  Run a forward or an
        integration first so the internal state holds finite data.  Returns a list of dicts."""
        lib, h = B.lib(), self._handle
        rows = C.c_int(0)
        lib.fc_unet_chains(h, C.byref(rows))
        batch = min(batch, rows.value)                 # launches are timed at no more than the reserved rows
        n = lib.fc_unet_plan_launches(h)
        ms = (C.c_float * n)()
        dev = self._handle_device
        B.check(lib.fc_unet_profile_ops(h, batch, repeats, ms, n, B.current_stream(dev)))
        out = []
        for i in range(n):
            k, m, f = C.c_char_p(), C.c_char_p(), C.c_double()
            B.check(lib.fc_unet_op_info(h, i, C.byref(k), C.byref(m), C.byref(f)))
            bp, bf = C.c_double(), C.c_double()
            B.check(lib.fc_unet_op_bytes(h, i, C.byref(bp), C.byref(bf)))
            out.append(dict(kernel=k.value.decode(), module=m.value.decode(), flops_per_sample=f.value, ms=float(ms[i]), rows=batch,
                            bytes=bp.value * batch + bf.value))
        return out

    def debug_tensor(self, name: str) -> torch.Tensor:
        """NHWC copy of an internal activation of the last forward (tests only)."""
        p, c, h, w = C.c_void_p(), C.c_int(), C.c_int(), C.c_int()
        B.check(B.lib().fc_unet_debug_tensor(self._handle, name.encode(), C.byref(p), C.byref(c), C.byref(h), C.byref(w)))
        return p.value, c.value, h.value, w.value
