"""Inpainting conditioning and its data: host-side mirror of ``flocoder/inpainting.py`` over the gfx950 library.

``MaskEncoder`` / ``mask_blending`` (inpainting.py:161-253) and ``algorithm3`` (inpainting.py:92-130), the training-free measurement
guidance the guided sampler applies (``sampling.generate_latents_guided``; on a ``flocoder_amd.Unet`` the correction runs inside the
library's RK4 stage kernels).

The mask generators and what feeds the mask-conditioned training path (inpainting.py:277-441): ``generate_mask``,
``generate_mask_batch``, ``create_inpainting_triplet``, ``InpaintingDataset`` under upstream's names, and ``InpaintingBatches``, the
batched producer of the dict batches ``preencode.process_dataset(inpainting=True)`` consumes.  The masks are counter-based
(``flocoder_amd.noise.mask_field`` is the definition and the NumPy form, ``fc_inpaint_masks`` in csrc/masks.hip the device form, equal in
every bit): a mask is a function of ``(seed, sample_id, size, type probabilities | forced type)``, so it is reproducible per sample
whatever the batch, the loader's workers or the rank -- upstream draws from the global ``np.random`` state.  Tensors come from the
device kernel; ``to_tensor=False`` returns the NumPy form and needs no GPU.  Upstream's cv2 brush variant, its plots and ``approx_AL``
stay out of scope."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch
from torch import nn
from torch.utils.data import IterableDataset

from . import _binding as B
from . import noise as N
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


# ---- mask generation and the training path's data (inpainting.py:277-441) ---------------------------------------------------------------
MASK_CHOICES = list(N.MASK_TYPES)
MASK_P = list(N.MASK_DEFAULT_P)
_NO_CPU = "flocoder_amd.{} runs on MI355X (gfx950) only; there is no CPU path (flocoder_amd.noise.mask_field is the NumPy form)"


def _device_masks(size, sample_ids, seed, device, choices, p, mask_type):
    """``fc_inpaint_masks``: (fp32 ``[B, 1, H, W]``, int32 ``[B]`` type codes) on ``device`` for the int64 ``sample_ids``."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(_NO_CPU.format("generate_mask"))
    h, w = (int(v) for v in size)
    ids = torch.as_tensor(sample_ids, dtype=torch.int64).reshape(-1).to(device).contiguous()     # ids made on the device are not copied
    if mask_type != "":
        if mask_type not in N.MASK_TYPES:
            raise ValueError(f"Unsupported mask_type: {mask_type}")
        forced, n, codes, probs = N.MASK_TYPES.index(mask_type), 0, None, None
    else:
        code_arr, _ = N.mask_type_thresholds(choices, p)             # validates as the host form does
        forced, n = -1, len(code_arr)
        codes = (ctypes.c_int * n)(*[int(c) for c in code_arr])
        probs = (ctypes.c_double * n)(*[float(v) for v in p])
    out = torch.empty(ids.numel(), 1, h, w, dtype=torch.float32, device=device)
    types = torch.empty(ids.numel(), dtype=torch.int32, device=device)
    B.check(B.lib().fc_inpaint_masks(B.ptr(out), B.ptr(types), int(seed) & 0xffffffffffffffff, B.ptr(ids), ids.numel(), h, w, codes, probs, n,
                                     forced, B.current_stream(device)))
    return out, types


def generate_mask(size=(128, 128), mask_type='', choices=MASK_CHOICES, p=MASK_P, to_tensor=True, device='cuda', *, seed=0, sample_id=0,
                  return_type=False):
    """inpainting.py:319-351, counter-based: the mask of ``(seed, sample_id)`` -- type drawn from ``choices`` with probabilities ``p`` unless
    ``mask_type`` names one -- as a ``[1, 1, H, W]`` fp32 tensor on ``device`` (made by the device kernel), or with ``to_tensor=False``
    as an ``[H, W]`` float64 array like upstream's (the NumPy form, bit-equal to the device's).  ``return_type`` adds the type's name."""
    if not to_tensor:
        m, t = N.mask_field(seed, [sample_id], size, choices, p, mask_type, return_types=True)
        m = m[0, 0].astype(np.float64)
        return (m, N.MASK_TYPES[int(t[0])]) if return_type else m
    m, t = _device_masks(size, [sample_id], seed, device, choices, p, mask_type)
    return (m, N.MASK_TYPES[int(t[0])]) if return_type else m


def generate_mask_batch(size=(128, 128), batch_size=1, unique_masks=False, to_tensor=True, *, seed=0, sample_ids=None, device='cuda', **kwargs):
    """inpainting.py:355-374: ``[batch_size, 1, H, W]`` masks (``[batch_size, H, W]`` array with ``to_tensor=False``).  With
    ``unique_masks`` row b is the mask of ``(seed, sample_ids[b])`` (ids ``0 .. batch_size-1`` by default); without, as upstream, ONE mask
    -- that of the first id -- tiled.  ``kwargs``: ``mask_type``, ``choices``, ``p``."""
    choices, p, mask_type = kwargs.pop("choices", MASK_CHOICES), kwargs.pop("p", MASK_P), kwargs.pop("mask_type", "")
    if kwargs:
        raise TypeError(f"generate_mask_batch: unexpected arguments {sorted(kwargs)}")
    if sample_ids is None:                                       # made where they are used: an upload from the host would wait for the stream
        sample_ids = torch.arange(int(batch_size), dtype=torch.int64, device=device if to_tensor else "cpu")
    ids = torch.as_tensor(sample_ids, dtype=torch.int64).reshape(-1)
    if not unique_masks:
        ids = ids[:1]
    elif ids.numel() != int(batch_size):
        raise ValueError(f"{ids.numel()} sample ids for batch_size={batch_size}")
    if not to_tensor:
        m = N.mask_field(seed, ids.cpu().numpy(), size, choices, p, mask_type)[:, 0].astype(np.float64)
        return m if unique_masks else np.tile(m, (int(batch_size), 1, 1))
    m, _ = _device_masks(size, ids, seed, device, choices, p, mask_type)
    return m if unique_masks else m.expand(int(batch_size), -1, -1, -1).contiguous()


def create_inpainting_triplet(full_image, codec, quantize=False, *, seed=0, sample_ids=None, **mask_kwargs):
    """inpainting.py:378-389, batched: ``(source_latents, mask_pixels, target_latents)`` for ``full_image`` ``[B, C, H, W]`` on the GPU --
    ``target = codec.encode(full_image)``, one mask per row (``sample_ids``, default ``0 .. B-1``), ``source = codec.encode(full_image *
    (1 - mask))``; ``quantize`` passes both through ``codec.quantize`` as upstream does."""
    if not full_image.is_cuda:
        raise RuntimeError(_NO_CPU.format("create_inpainting_triplet"))
    bsz = full_image.shape[0]
    target_latents = codec.encode(full_image)
    mask_pixels = generate_mask_batch(tuple(full_image.shape[-2:]), bsz, unique_masks=True, seed=seed, sample_ids=sample_ids,
                                      device=full_image.device, **mask_kwargs)
    source_latents = codec.encode(full_image * (1 - mask_pixels))
    if quantize:
        source_latents, target_latents = codec.quantize(source_latents), codec.quantize(target_latents)
    return source_latents, mask_pixels, target_latents


def _split_item(item):
    if isinstance(item, (tuple, list)):
        return item[0], (item[1] if len(item) > 1 else 0)
    return item, 0


class InpaintingDataset(IterableDataset):
    """inpainting.py:411-441: wraps a dataset of GPU images (or ``(image, label)`` items) and yields upstream's per-item dict
    ``{'source_image', 'mask_pixels' [H, W], 'target_image', 'label'}``.  The mask of an item is that of ``(seed, running item index)``;
    ``mask_kwargs``: ``mask_type``, ``choices``, ``p``."""

    def __init__(self, base_dataset, mask_kwargs=None, *, seed=0):
        self.base_dataset, self.mask_kwargs, self.seed = base_dataset, dict(mask_kwargs or {}), seed
        if hasattr(base_dataset, 'actual_len'):
            self.actual_len = base_dataset.actual_len

    def __iter__(self):
        for index, item in enumerate(self.base_dataset):
            full_image, label = _split_item(item)
            if not full_image.is_cuda:
                raise RuntimeError(_NO_CPU.format("InpaintingDataset"))
            mask_pixels = generate_mask(size=tuple(full_image.shape[-2:]), device=full_image.device, seed=self.seed, sample_id=index,
                                        **self.mask_kwargs).squeeze()
            yield {'source_image': full_image * (1 - mask_pixels), 'mask_pixels': mask_pixels, 'target_image': full_image, 'label': label}


class InpaintingBatches:
    """Wraps any loader of ``(images, classes)`` batches and yields the dict batches ``preencode.process_dataset(inpainting=True)``
    consumes: ``{'source_image' [B,C,H,W], 'mask_pixels' [B,1,H,W], 'target_image' [B,C,H,W], 'label'}``, images moved to ``device``,
    masks and masked images made there.  The sample id of an item is its global index in the loader's order (``first_id`` + items before
    it), so every rank that walks the same loader sees the same mask on the same item whichever batches it goes on to encode."""

    def __init__(self, loader, seed=0, device='cuda', first_id=0, **mask_kwargs):
        self.loader, self.seed, self.device, self.first_id, self.mask_kwargs = loader, seed, torch.device(device), int(first_id), mask_kwargs
        if self.device.type != "cuda":
            raise RuntimeError(_NO_CPU.format("InpaintingBatches"))

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        next_id = self.first_id
        for batch in self.loader:
            images, classes = _split_item(batch)
            images = images.to(self.device, non_blocking=True)
            bsz = images.shape[0]
            ids = torch.arange(next_id, next_id + bsz, dtype=torch.int64, device=self.device)
            next_id += bsz
            mask_pixels = generate_mask_batch(tuple(images.shape[-2:]), bsz, unique_masks=True, seed=self.seed, sample_ids=ids,
                                              device=self.device, **self.mask_kwargs)
            yield {'source_image': images * (1 - mask_pixels), 'mask_pixels': mask_pixels, 'target_image': images, 'label': classes}
