"""Inpainting conditioning: host-side mirror of ``flocoder/inpainting.py``'s ``MaskEncoder`` / ``mask_blending``
(inpainting.py:161-253) over the gfx950 library, and ``algorithm3`` (inpainting.py:92-130), the training-free measurement guidance the
guided sampler applies (``sampling.generate_latents_guided``; on a ``flocoder_amd.Unet`` the correction runs inside the library's RK4
stage kernels).  The mask *generators*, ``InpaintingDataset`` and the diagnostics of that file are data preparation and stay out of
scope."""
from __future__ import annotations

import math

import torch
from torch import nn

from . import _binding as B
from ._native import NativeModule


class _MaskEncoderFunction(torch.autograd.Function):
    """Autograd bridge for MaskEncoder training (train_flow.py:312-318,361-371).  The reference calls the encoder three times per
    step (the batch's masks, all ones, all zeros) before ``loss.backward()``; the native object keeps the activations of its LAST
    forward only, so the backward re-runs the (3 MFLOP) forward of its own call first."""

    @staticmethod
    def forward(ctx, model, x, *params):
        ctx.model = model
        ctx.save_for_backward(x)
        return model._forward_native(x)

    @staticmethod
    def backward(ctx, d_out):
        (x,) = ctx.saved_tensors
        model = ctx.model
        flat = model.backward_native(x, d_out)
        return (None, None, *[flat[off:off + math.prod(shape)].view(shape).clone() for _, shape, off in model._table])


class MaskEncoder(NativeModule):
    """inpainting.py:182-245 with the defaults the flow trainer uses (output_channels=4, shrink_fac=4, mode='pool', sigmoid):
    pixel mask [B,1,H,W] -> [B,4,H/16,W/16]; channel 0 is the 16x average-pooled raw mask, channels 1-3 are learned.
    Same ``state_dict`` keys as upstream (``layers.0.conv1.weight`` ...) and the same default init / RNG order."""

    _fc = "fc_mask_encoder"

    def __init__(self, output_channels=4, shrink_fac=4, mode='pool', final_act=torch.sigmoid):
        super().__init__()
        if output_channels != 4 or shrink_fac != 4 or mode != 'pool':
            raise NotImplementedError("only the configuration train_flow.py instantiates (MaskEncoder()) is built")
        self._read_table()
        self._register_table()                                 # registration order = upstream construction order
        with torch.no_grad():                                  # nn.Conv2d defaults, weight then bias
            for name, shape, _ in self._table:
                p = self.get_parameter(name)
                if len(shape) > 1:
                    nn.init.kaiming_uniform_(p, a=math.sqrt(5))
                    fan_in = math.prod(shape[1:])
                else:
                    p.uniform_(-1.0 / math.sqrt(fan_in), 1.0 / math.sqrt(fan_in))

    def forward(self, mask_pixels):
        if not mask_pixels.is_cuda:
            raise RuntimeError("flocoder_amd.MaskEncoder runs on MI355X (gfx950) only; there is no CPU path")
        if mask_pixels.dtype in (torch.uint8, torch.int32, torch.int64, torch.bool):      # inpainting.py:236-237
            mask_pixels = mask_pixels.float()
        x = mask_pixels.detach().contiguous().float()
        if x.shape[1] != 1:
            raise ValueError("mask_pixels must have one channel")
        if torch.is_grad_enabled() and self.training and any(p.requires_grad for p in self.parameters()):
            return _MaskEncoderFunction.apply(self, x, *[self.get_parameter(n) for n, _, _ in self._table])
        with torch.no_grad():
            return self._forward_native(x)

    def _forward_native(self, x):
        bsz, _, h, w = x.shape
        hnd = self._native(x.device)
        B.check(B.lib().fc_mask_encoder_reserve(hnd, bsz, h, w))
        out = torch.empty(bsz, 4, h // 16, w // 16, device=x.device)
        B.check(B.lib().fc_mask_encoder_forward(hnd, B.ptr(x), B.ptr(out), bsz, h, w, B.current_stream(x.device)))
        return out

    def backward_native(self, x, d_out, grads=None, accumulate=False):
        """Parameter gradients (flat, table layout) for d(mask_latents) = ``d_out`` of the forward on ``x`` -- which is re-run first."""
        bsz, _, h, w = x.shape
        out = self._forward_native(x)
        if grads is None:
            grads = torch.zeros(self._flat_numel, device=x.device)
            accumulate = False
        B.check(B.lib().fc_mask_encoder_backward(self._native(x.device), B.ptr(x), B.ptr(out), B.ptr(d_out.contiguous().float()), B.ptr(grads),
                                                 grads.numel(), int(accumulate), bsz, h, w, B.current_stream(x.device)))
        return grads

    def grad_views(self, flat):
        return {name: flat[off:off + math.prod(shape)].view(shape) for name, shape, off in self._table}


def mask_blending(source, mask, noise=None):
    """inpainting.py:250-253: source + mask*(noise - source)."""
    if noise is None:
        noise = torch.randn_like(source)
    if not source.is_cuda:
        raise RuntimeError("flocoder_amd.mask_blending runs on MI355X (gfx950) only; there is no CPU path")
    if torch.is_grad_enabled() and any(t.requires_grad for t in (source, mask, noise)):
        return source + mask * (noise - source)             # under autograd (MaskEncoder training): three device elementwise ops on a latent
    s, m, n = (t.contiguous().float() for t in (source, mask.expand_as(source), noise))
    out = torch.empty_like(s)
    B.check(B.lib().fc_mask_blend(B.ptr(s), B.ptr(m), B.ptr(n), B.ptr(out), s.numel(), B.current_stream(s.device)))
    return out


def guidance_weight(v, x, tp, y, a, sigma_y=0.05):
    """``w = a (y - a x1) / (r2 a^2 + sigma_y^2)`` with ``x1 = x + (1 - tp) v`` and ``r2 = (1-tp)^2 / (tp^2 + (1-tp)^2)``: algorithm3's
    ``(y - A x1)^T (r2 A A^T + sigma_y^2 I)^-1 A`` for the diagonal operator ``A = diag(a)`` (``a`` of x's shape or broadcastable to it),
    elementwise and batched; 0 where the denominator is 0 (``a = 0`` with ``sigma_y = 0``: nothing is measured there)."""
    om = 1 - tp
    x1 = x + om * v
    r2 = om ** 2 / (tp ** 2 + om ** 2)
    den = r2 * (a * a) + sigma_y ** 2
    num = a * (y - a * x1)
    return torch.where(den == 0, torch.zeros_like(num), num / torch.where(den == 0, torch.ones_like(den), den))


def algorithm3(v, x, t, tp, y, A, sigma_y=0.05, gamma_t=1.0):
    """inpainting.py:92-130, "solve inverse problems via flows with a pretrained vector field" on the conditional-OT path (alpha_t = t,
    sigma_t = 1 - t): the velocity ``v`` a pretrained flow gives at ``(x, tp)`` corrected so that the trajectory agrees with the
    measurement ``y = A x_1``.  ``t`` is accepted for signature parity (upstream never reads it).  With the upstream coefficients
    reduced -- ``(alpha d ln(alpha/sigma)/dt)^-1 = 1 - tp``, ``sigma^2 d ln(alpha/sigma)/dt = (1 - tp)/tp`` -- no intermediate is singular:

        x1 = x + (1 - tp) v        g = (y - A x1)^T (r2 A A^T + sigma_y^2 I)^-1 A        v_c = v + gamma_t ((1 - tp)/tp) g

    (d x1 / d x is taken as the identity, as upstream; ``sampling.generate_latents_guided(jacobian="exact")`` adds the rest.)  ``A`` is
    either a dense ``[k, n]`` matrix -- one flattened sample of n elements, ``y`` of k, the ``k x k`` solve of upstream -- or a tensor of
    x's shape / ``[B,1,H,W]``: the diagonal operator, for which the solve is the elementwise ``guidance_weight``, batched.  Finite for
    ``0 < tp <= 1`` (at ``tp = 1`` the result is ``v``); ``tp <= 0`` raises ValueError (upstream returns NaN at both ends)."""
    if not float(tp) > 0:
        raise ValueError(f"algorithm3: tp={float(tp)} must be > 0 (the correction carries the factor (1 - tp)/tp)")
    om = 1 - tp
    coef = gamma_t * om / tp
    if A.dim() == 2 and A.shape[1] == x.numel() and tuple(A.shape) != tuple(x.shape):      # the dense form
        x1 = x + om * v
        r2 = om ** 2 / (tp ** 2 + om ** 2)
        residual = y - A @ x1.flatten()
        cov = r2 * (A @ A.T) + sigma_y ** 2 * torch.eye(A.shape[0], device=x.device, dtype=A.dtype)
        g = (residual @ torch.linalg.solve(cov, A)).view_as(x)
    else:
        g = guidance_weight(v, x, tp, y, A, sigma_y)
    return v + coef * g
