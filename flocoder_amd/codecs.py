"""Codec plugin API: host-side mirror of ``flocoder/codecs.py``'s factory and codec wrappers (codecs.py:578-741).

``setup_codec(config, device, no_natten=False, load_checkpoint=True, eval=True)`` returns an object with the protocol the
flow path consumes: ``encode(x) -> z``, ``decode(z, orig_size=None, noise_strength=0.0) -> x``,
``forward(x, noise_strength, minval, get_stats)``, ``in_channels``, ``parameters()``.  The SD codec runs on the gfx950
library (``fc_vae_*``) and the VQVAE's encode / decode on ``fc_vqvae_*``; there is no CPU path for either.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, Optional

import torch
import torch.nn.functional as F
from torch import nn

from . import _binding as B
from ._native import NativeModule, _Node, read_param_table
from .general import ldcfg


class SimpleResizeAE(nn.Module):
    """codecs.py:578-619 -- interpolation 'codec' (encode: resize to latent_shape, extra channels = channel mean)."""

    def __init__(self, in_channels=3, latent_shape=(4, 16, 16), mode='bicubic'):
        super().__init__()
        self.in_channels, self.latent_shape, self.orig_shape, self.mode = in_channels, latent_shape, None, mode

    def encode(self, x):
        self.orig_shape = x.shape[1:]
        if self.latent_shape is None or self.orig_shape == self.latent_shape:
            return x
        c, h, w = self.latent_shape
        small = F.interpolate(x, size=(h, w), mode=self.mode, align_corners=False)
        if c == x.shape[-3]:
            return small
        return torch.cat([small, small.mean(dim=1, keepdim=True).repeat(1, c - x.shape[-3], 1, 1)], dim=1)

    def decode(self, z, orig_shape=None, noise_strength=0.0):
        target = orig_shape if orig_shape is not None else self.orig_shape
        if self.latent_shape is None or target is None or target == self.latent_shape:
            return z
        return F.interpolate(z[:, :3], size=(target[-2], target[-1]), mode=self.mode, align_corners=False)

    def forward(self, x, noise_strength=0.0, minval=0, get_stats=False):
        recon = self.decode(self.encode(x))
        return (recon, 0.0, {'codebook_mean_dist': 0.0, 'codebook_max_dist': 0.0}) if get_stats else (recon, 0.0)


class NoOpAE(SimpleResizeAE):
    """codecs.py:621-627.  As upstream, the parent constructor resets latent_shape to (4,16,16), so 'noop' resizes
     -- kept, because checkpoints trained against that behaviour expect it."""

    def __init__(self):
        self.latent_shape = None
        super().__init__()


# legacy (pre-0.14 diffusers) attention parameter names still present in the published sd-vae-ft-mse checkpoint
_LEGACY = {".query.": ".to_q.", ".key.": ".to_k.", ".value.": ".to_v.", ".proj_attn.": ".to_out.0."}


def vae_param_table():
    """(name, shape, offset) of the native AutoencoderKL parameter table, and its flat numel (no GPU needed)."""
    return read_param_table("fc_vae", "create")


_PRECISIONS = {"fp32": 0, "bf16x3": 1}


class _NativeCodec(NativeModule):
    """What the two native codecs share: precision, the reserve-then-run body of encode / decode, and the plan tables."""

    def set_precision(self, mode: str = "fp32") -> None:
        """Arithmetic of the codec's convolutions: "fp32" (default, exact fp32 on the matrix pipe -- what parity tests and the headline use)
        or "bf16x3" (every operand as bf16 hi + lo, three bf16 MFMAs per product, fp32 accumulation: ~1e-5 relative per layer; an opt-in for
        callers that decode many images, ``<codec>_set_precision``)."""
        if mode not in _PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_PRECISIONS)}")
        self._precision = mode

    def debug_taps(self, on: bool = True) -> None:
        """Tests only: plans built from now on recycle no activation buffer and record every module's tensors by name (``debug_tensor``).
        Switching drops the plans in place; off (the default) is the ordinary recycled plan."""
        self._taps = bool(on)

    def debug_tensor(self, name: str, decode: bool = True):
        """(device pointer, C, H, W) of the NHWC tensor the last encode / decode left under ``name`` (``_ops.fetch_tap`` copies it)."""
        p, c, h, w = C.c_void_p(), C.c_int(), C.c_int(), C.c_int()
        B.check(self._fn("debug_tensor")(self._handle, int(decode), name.encode(), C.byref(p), C.byref(c), C.byref(h), C.byref(w)))
        return p.value, c.value, h.value, w.value

    def _on_use(self, handle, device):
        B.check(self._fn("set_precision")(handle, _PRECISIONS[getattr(self, "_precision", "fp32")]))
        B.check(self._fn("debug_taps")(handle, int(getattr(self, "_taps", False))))

    def _need_gpu(self, t):
        if not t.is_cuda:
            raise RuntimeError(f"flocoder_amd.{type(self).__name__} runs on MI355X (gfx950) only; there is no CPU path")

    def _run(self, op: str, x, out_shape):
        """``op`` = "encode" | "decode" of the GPU tensor ``x`` into a new fp32 tensor of ``out_shape``, the plan reserved for x's shape first."""
        bsz, _, h, w = x.shape
        x = x.contiguous().float()
        hnd = self._native(x.device)
        B.check(self._fn("reserve_" + op)(hnd, bsz, h, w))
        out = torch.empty(out_shape, device=x.device, dtype=torch.float32)
        B.check(self._fn(op)(hnd, B.ptr(x), B.ptr(out), bsz, h, w, B.current_stream(x.device)))
        return out

    def flops_per_sample(self, decode=True) -> float:
        return float(self._fn("flops_per_sample")(self._handle, int(decode))) if self._handle else 0.0

    def _op_record(self, decode, i):
        """(kernel family, reference module, FLOPs per sample, HBM bytes per sample, HBM bytes per launch) of launch i of a plan."""
        raise NotImplementedError

    def _plan_records(self, decode):
        n = self._fn("plan_launches")(self._handle, int(decode)) if self._handle else 0
        return [self._op_record(decode, i) for i in range(n)]

    def plan_ops(self, decode=True):
        """(kernel family, reference module, algorithmic FLOPs per sample) of every launch of the current decode / encode plan."""
        return [r[:3] for r in self._plan_records(decode)]

    def plan_kernels(self, decode=True):
        return [k for k, _, _ in self.plan_ops(decode)]

    def profile_ops(self, inp: torch.Tensor, out: torch.Tensor, decode=True, repeats: int = 5):
        """Per-launch device milliseconds of the decode (or encode) plan for the batch ``inp`` -> ``out`` with each launch's kernel
        family, algorithmic FLOPs per sample and algorithmic HBM bytes (bench.py's live roofline measurement for the codecs).  Run
        decode()/encode() at this batch first so the plan exists."""
        recs = self._plan_records(decode)
        ms = (C.c_float * max(len(recs), 1))()
        B.check(self._fn("profile_ops")(self._handle, int(decode), B.ptr(inp.contiguous()), B.ptr(out), inp.shape[0], repeats, ms, len(recs),
                                        B.current_stream(inp.device)))
        return [dict(kernel=k, module=m, flops_per_sample=f, ms=float(ms[i]), rows=inp.shape[0], bytes=bp * inp.shape[0] + bf)
                for i, (k, m, f, bp, bf) in enumerate(recs)]


class SD_VAE_Wrapper(_NativeCodec):
    """codecs.py:631-663 over the native AutoencoderKL.  Parameters live under ``self.vae.*`` with the upstream key names, so a
    ``state_dict`` saved from the reference's wrapper loads here unchanged.

    The reference calls ``AutoencoderKL.from_pretrained("stabilityai/sd-vae-ft-mse")`` (a network fetch).  Here weights come from a
    LOCAL copy: ``weights`` = a state_dict, a ``.safetensors`` / ``.pt`` file, or a directory holding
    ``diffusion_pytorch_model.safetensors`` (also taken from ``$FLOCODER_SD_VAE_PATH``); ``weights="random"`` draws seeded random
    weights (benchmarks / tests).  Without any of these it raises FileNotFoundError -- it never downloads."""

    _fc = "fc_vae"

    def __init__(self, pretrained_model_name="stabilityai/sd-vae-ft-mse", weights=None, seed: int = 0):
        super().__init__()
        self.in_channels = 3
        self.pretrained_model_name = pretrained_model_name
        self._read_table()
        self.vae = _Node()
        self._register_table(requires_grad=False)
        if weights is None:
            weights = os.environ.get("FLOCODER_SD_VAE_PATH")
        if weights is None:
            raise FileNotFoundError(
                f"SD_VAE_Wrapper: no local weights for '{pretrained_model_name}'. Pass weights=<dir|file|state_dict> or set "
                "FLOCODER_SD_VAE_PATH (the reference downloads them; this build never touches the network).")
        if isinstance(weights, str) and weights == "random":
            self._init_random(seed)
        else:
            self.load_vae_state_dict(weights if isinstance(weights, dict) else _read_weights(weights))

    # ---- weights
    def _init_random(self, seed):
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for name, p in self.vae.named_parameters():
                leaf = name.rsplit(".", 1)[1]
                if p.dim() == 1:
                    p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g) if leaf == "weight" else 0.05 * torch.randn(p.shape, generator=g))
                else:
                    p.copy_(torch.randn(p.shape, generator=g) * (1.0 / math.prod(p.shape[1:])) ** 0.5)

    def load_vae_state_dict(self, sd: Dict[str, torch.Tensor]):
        sd = dict(sd)
        for k in list(sd):
            nk = k[4:] if k.startswith("vae.") else k
            for old, new in _LEGACY.items():
                nk = nk.replace(old, new)
            if nk != k:
                sd[nk] = sd.pop(k)
        own = dict(self.vae.named_parameters())
        missing = [k for k in own if k not in sd]
        if missing:
            raise KeyError(f"SD-VAE weights are missing {len(missing)} tensors, e.g. {missing[:3]}")
        with torch.no_grad():
            for k, p in own.items():
                p.copy_(sd[k].reshape(p.shape).to(p.dtype))      # legacy attention weights are [C,C,1,1]
        self.mark_dirty()

    @property
    def _root(self):
        return self.vae

    # ---- codec protocol
    @torch.no_grad()
    def encode(self, x):
        """vae.encode(x).latent_dist.mean.detach() (codecs.py:639-642): deterministic, no 0.18215 scaling."""
        self._need_gpu(x)
        bsz, ch, h, w = x.shape
        if ch != 3:
            raise ValueError("SD-VAE expects 3-channel images")
        return self._run("encode", x, (bsz, 4, h // 8, w // 8))

    @torch.no_grad()
    def decode(self, z, orig_size=None, noise_strength=0.0):
        """vae.decode(z).sample (codecs.py:649-652)."""
        self._need_gpu(z)
        bsz, ch, h, w = z.shape
        if ch != 4:
            raise ValueError("SD-VAE latents have 4 channels")
        return self._run("decode", z, (bsz, 3, 8 * h, 8 * w))

    def forward(self, x, noise_strength=0.0, minval=0, get_stats=False):
        """codecs.py:657-663."""
        self.last_min, self.last_max = x.min(), x.max()
        recon = self.decode(self.encode(x))
        return (recon, 0.0, {'codebook_mean_dist': 0.0, 'codebook_max_dist': 0.0}) if get_stats else (recon, 0.0)

    def _op_record(self, decode, i):
        lib, h = B.lib(), self._handle
        k, m, f, bp, bf = C.c_char_p(), C.c_char_p(), C.c_double(), C.c_double(), C.c_double()
        B.check(lib.fc_vae_op_info(h, int(decode), i, C.byref(k), C.byref(m), C.byref(f)))
        B.check(lib.fc_vae_op_bytes(h, int(decode), i, C.byref(bp), C.byref(bf)))
        return k.value.decode(), m.value.decode(), f.value, bp.value, bf.value


class _NoiseInjectionParams(nn.Module):
    """Parameter holder for NoiseInjection (codecs.py:217-241): a no-op at noise_strength 0, which is all the flow path uses;
    the tensors exist so reference checkpoints round-trip through ``state_dict``."""

    def __init__(self, channels):
        super().__init__()
        self.to_noise_scale = nn.Conv2d(channels, channels, 1)
        self.to_noise_bias = nn.Conv2d(channels, channels, 1)
        nn.init.zeros_(self.to_noise_scale.weight)
        nn.init.zeros_(self.to_noise_bias.weight)


class _Codebook(nn.Module):
    def __init__(self, size, dim):
        super().__init__()
        self.register_buffer("initted", torch.tensor(False))
        self.register_buffer("cluster_size", torch.zeros(1, size))
        self.register_buffer("embed_avg", torch.zeros(1, size, dim))
        self.register_buffer("embed", torch.zeros(1, size, dim))


class _VQLayer(nn.Module):
    def __init__(self, size, dim):
        super().__init__()
        self._codebook = _Codebook(size, dim)


class ResidualVQ(nn.Module):
    """``vector_quantize_pytorch.ResidualVQ`` as VQVAE builds it (codecs.py:456-467), holding the buffers under the package's state_dict
    names (``layers.{i}._codebook.{initted,cluster_size,embed_avg,embed}``) so trained checkpoints load.  THIRD-PARTY ALGORITHM, PARITY
    UNPINNED (the package is absent offline): per level the nearest codeword of the running residual, output = their sum.

    Eval mode is the inference form (``fc_rvq_quantize``): codebooks that were never initialised (``initted`` false) raise, the losses
    are zero.  Training mode FITS the codebooks on the device, without gradients (``fc_rvq_train_step``; the definition is
    ``flocoder_amd/noise.py``, "codebook fitting"): a level whose ``initted`` is false is first initialised from the batch -- ``codebook_size``
    drawn residual vectors, then ``kmeans_iters`` Lloyd iterations (none with ``kmeans_init=False``) --, then every level assigns against
    its current codebook and updates ``cluster_size`` / ``embed_avg`` / ``embed`` by the EMA rule with ``decay`` and replaces codes whose
    cluster size fell below ``threshold_ema_dead_code``.  A training call returns ``(quantized, indices, losses [1, levels])`` from the
    PRE-update codebooks, the losses ``commitment_weight`` * mean squared distance per level.  THE OUTPUTS CARRY NO GRADIENT: neither the
    straight-through / rotation-trick path to the encoder nor the orthogonality term (which acts only through the gradients of a
    learnable codebook; EMA codebooks have none) is built.  ``seed`` and ``draw_index`` (advanced once per training call) select the
    counter-based draws; they are plain attributes, not buffers: a caller that wants a resumed run to replay the draws carries them.
    ``last_expired`` holds the last training call's expired codes per level (int32, on the device)."""

    def __init__(self, dim, codebook_size, num_quantizers, decay=0.95, commitment_weight=0.25, kmeans_init=True, kmeans_iters=15,
                 threshold_ema_dead_code=2, seed=0, **unused):
        super().__init__()
        self.dim, self.codebook_size, self.num_quantizers = dim, codebook_size, num_quantizers
        self.decay, self.commitment_weight = float(decay), float(commitment_weight)
        self.kmeans_init, self.kmeans_iters = bool(kmeans_init), int(kmeans_iters)
        self.threshold_ema_dead_code = float(threshold_ema_dead_code)
        self.seed, self.draw_index, self.last_expired = int(seed), 0, None
        self.layers = nn.ModuleList([_VQLayer(codebook_size, dim) for _ in range(num_quantizers)])

    @property
    def codebooks(self):
        return torch.stack([l._codebook.embed[0] for l in self.layers])

    def _check(self, t):
        if not all(bool(l._codebook.initted) for l in self.layers):
            raise NotImplementedError("ResidualVQ: codebooks are uninitialised (k-means init is not built); load a trained checkpoint")
        self._need_gpu(t)

    @staticmethod
    def _need_gpu(t):
        if not t.is_cuda:
            raise RuntimeError("flocoder_amd.ResidualVQ runs on MI355X (gfx950) only; there is no CPU path")

    @torch.no_grad()
    def _fit_nchw(self, z):
        """One training call on z [B, dim, h, w]: initialise what is not, then the step.  One host read (``initted``), no other wait."""
        self._need_gpu(z)
        bsz, d, h, w = z.shape
        z = z.detach().contiguous().float()
        lib, dev, nl, k = B.lib(), z.device, self.num_quantizers, self.codebook_size
        nbytes = lib.fc_rvq_train_workspace_bytes(bsz, h * w, d, k, nl)
        if not nbytes:
            raise ValueError(f"flocoder_amd: {lib.fc_last_error().decode(errors='replace')}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        books = [l._codebook for l in self.layers]
        cb = torch.stack([c.embed[0] for c in books]).to(dev).contiguous()
        cs = torch.stack([c.cluster_size[0] for c in books]).to(dev).contiguous()
        ea = torch.stack([c.embed_avg[0] for c in books]).to(dev).contiguous()
        initted = torch.stack([c.initted for c in books]).tolist()
        shape, stream, draw = (bsz, d, h * w, k, nl), B.current_stream(dev), self.draw_index & 0xffffffff
        for lvl, done in enumerate(initted):               # in sequence: level l's residuals need the finished level l - 1
            if done:
                continue
            B.check(lib.fc_rvq_seed_codes(B.ptr(z), B.ptr(cb), *shape, lvl, self.seed, draw, stream))
            B.check(lib.fc_rvq_kmeans(B.ptr(z), B.ptr(cb), *shape, lvl, self.kmeans_iters if self.kmeans_init else 0, B.ptr(cs[lvl]),
                                      B.ptr(ea[lvl]), None, B.ptr(ws), nbytes, stream))
        zq = torch.empty_like(z)
        idx = torch.empty(bsz * h * w, nl, dtype=torch.int64, device=dev)
        losses = torch.empty(nl, dtype=torch.float32, device=dev)
        expired = torch.empty(nl, dtype=torch.int32, device=dev)
        B.check(lib.fc_rvq_train_step(B.ptr(z), B.ptr(cb), B.ptr(cs), B.ptr(ea), B.ptr(zq), B.ptr(idx), B.ptr(losses), B.ptr(expired), *shape,
                                      self.decay, self.commitment_weight, self.threshold_ema_dead_code, self.seed, draw, B.ptr(ws), nbytes, stream))
        for lvl, c in enumerate(books):
            c.embed[0].copy_(cb[lvl])
            c.cluster_size[0].copy_(cs[lvl])
            c.embed_avg[0].copy_(ea[lvl])
            c.initted.fill_(True)
        self.draw_index += 1
        self.last_expired = expired
        return zq, idx, losses.view(1, nl)

    def quantize_nchw(self, z):
        if self.training:
            return self._fit_nchw(z)
        self._check(z)
        bsz, d, h, w = z.shape
        z = z.contiguous().float()
        cb = self.codebooks.to(z.device).contiguous()
        zq = torch.empty_like(z)
        idx = torch.empty(bsz * h * w, self.num_quantizers, dtype=torch.int64, device=z.device)
        B.check(B.lib().fc_rvq_quantize(B.ptr(z), B.ptr(cb), B.ptr(zq), B.ptr(idx), bsz, d, h * w, self.codebook_size, self.num_quantizers,
                                        B.current_stream(z.device)))
        return zq, idx, torch.zeros(1, self.num_quantizers, device=z.device)

    def forward(self, x):
        """x [N, dim] (as VQVAE.quantize passes it) or [B, n, dim] -> (quantized, indices [..., levels], losses [1, levels])."""
        flat = x.reshape(-1, x.shape[-1])
        zq, idx, loss = self.quantize_nchw(flat.t().contiguous().view(1, x.shape[-1], flat.shape[0], 1))
        return zq.view(x.shape[-1], flat.shape[0]).t().reshape(x.shape), idx.view(*x.shape[:-1], self.num_quantizers), loss


class VQVAE(_NativeCodec):
    """codecs.py:395-574 -- encode / decode on the gfx950 library (``fc_vqvae_*``), NATTEN-less, eval mode.

    Parameters carry the reference's state_dict names (``encoder.0.conv1.weight`` ... ``decoder.layers.0.q_proj.weight`` ...), so
    ``load_state_dict(ckpt['model_state_dict'], strict=False)`` takes a reference checkpoint as is.  ``quantize`` / ``forward`` run the
    inference form of ResidualVQ (third party, parity unpinned -- see ``ResidualVQ`` above); ``fit_codebooks`` fits the codebooks to the
    encoder's latents without gradients; ``forward`` in training mode (codec training through the encoder) and ``decode`` with a non-zero
    ``noise_strength`` (training-time NoiseInjection) raise NotImplementedError."""

    _fc, _create = "fc_vqvae", "create_ex"

    def __init__(self, in_channels=3, hidden_channels=256, num_downsamples=3, vq_num_embeddings=512, internal_dim=256,
                 codebook_levels=3, vq_embedding_dim=4, commitment_weight=0.25, use_checkpoint=False, no_natten=False,
                 encoder_nonlocal=False, decoder_nonlocal=True, natten_layout=0):
        """``natten_layout``: 0 = no NATTENBlocks (what the reference builds when the natten package is missing or ``no_natten``),
        1 / 2 = with them (needed to load a checkpoint TRAINED with NATTEN): 1 reads the 7x7 windows over image rows x
        columns per head, 2 reproduces what natten >= 0.20 makes of the reference's [B, heads, H, W, d] call (include/flocoder_amd.h,
        fc_vqvae_create_ex).  Third-party arithmetic, parity unpinned."""
        super().__init__()
        if encoder_nonlocal:
            raise NotImplementedError("VQVAE(encoder_nonlocal=True) is not built (no reference config uses it)")
        natten_layout = 0 if no_natten else int(natten_layout)
        self.in_channels, self.num_downsamples = in_channels, num_downsamples
        self.codebook_levels, self.vq_num_embeddings = codebook_levels, vq_num_embeddings
        self.vq_embedding_dim, self.indices, self.info = vq_embedding_dim, None, None
        self._cfg = (in_channels, hidden_channels, num_downsamples, internal_dim, vq_embedding_dim, int(bool(decoder_nonlocal)), natten_layout)
        self.natten_layout = natten_layout
        self._read_table()
        self._register_table(requires_grad=False)
        with torch.no_grad():
            for name, shape, _ in self._table:
                p, leaf = self.get_parameter(name), name.rsplit(".", 1)[1]
                if leaf == "gamma":
                    p.zero_()                                             # NATTENBlock's residual gate starts closed (codecs.py:105)
                elif name.endswith((".attn.qkv.weight", ".attn.proj.weight")):
                    p.normal_(0.0, 0.02)                                  # codecs.py:108-109
                elif leaf == "weight" and len(shape) > 1:                 # nn.Conv2d default init (kaiming_uniform, a=sqrt(5))
                    nn.init.kaiming_uniform_(p, a=math.sqrt(5))
                elif leaf == "weight":
                    p.fill_(1.0)                                          # GroupNorm
                else:
                    wname = name[:-4] + "weight"
                    wshape = next(s for n, s, _ in self._table if n == wname)
                    bound = 1.0 / math.sqrt(math.prod(wshape[1:])) if len(wshape) > 1 else 0.0
                    p.uniform_(-bound, bound) if bound else p.zero_()
        # NoiseInjection tensors of the reference's Decoder (codecs.py:259,283-300): present in checkpoints, unused at strength 0
        i0 = 1 if decoder_nonlocal else 0
        cur = hidden_channels * 2 ** (num_downsamples - 1)
        self.decoder.layers.add_module(str(i0 + 4), _NoiseInjectionParams(cur))
        i = i0 + 6
        for lvl in range(num_downsamples - 1, -1, -1):
            co = hidden_channels * 2 ** max(0, lvl - 1) if lvl else hidden_channels
            self.decoder.layers.add_module(str(i + 3), _NoiseInjectionParams(cur))
            self.decoder.layers.add_module(str(i + 5), _NoiseInjectionParams(co))
            cur, i = co, i + 7
        self.decoder.layers.add_module(str(i), _NoiseInjectionParams(cur))
        self.decoder.layers.add_module(str(i + 3), _NoiseInjectionParams(64))
        self.vq = ResidualVQ(dim=vq_embedding_dim, codebook_size=vq_num_embeddings, num_quantizers=codebook_levels, decay=0.95,
                             commitment_weight=commitment_weight, kmeans_init=True, kmeans_iters=15, threshold_ema_dead_code=2)
        self.register_buffer('codebook_usage', torch.zeros(codebook_levels, vq_num_embeddings))
        self.usage_count = 0

    def _create_args(self):
        return self._cfg

    @torch.no_grad()
    def encode(self, x, debug=False):
        """z = self.encoder(x) (codecs.py:492-502): [B,in_channels,H,W] -> [B,vq_embedding_dim,H>>nd,W>>nd], pre-quantisation."""
        self._need_gpu(x)
        bsz, ch, h, w = x.shape
        if ch != self.in_channels:
            raise ValueError(f"VQVAE expects {self.in_channels}-channel input, got {ch}")
        nd = self.num_downsamples
        return self._run("encode", x, (bsz, self.vq_embedding_dim, h >> nd, w >> nd))

    @torch.no_grad()
    def decode(self, z_q, noise_strength=0.0):
        """self.decoder(z_q, noise_strength) (codecs.py:523-525) at noise_strength 0."""
        if noise_strength:
            raise NotImplementedError("VQVAE.decode: noise_strength != 0 (training-time NoiseInjection) is not built")
        self._need_gpu(z_q)
        bsz, ch, h, w = z_q.shape
        if ch != self.vq_embedding_dim:
            raise ValueError(f"VQVAE latents have {self.vq_embedding_dim} channels, got {ch}")
        nd = self.num_downsamples
        return self._run("decode", z_q, (bsz, self.in_channels, h << nd, w << nd))

    def quantize(self, z, debug=False):
        """codecs.py:504-521: z [B,C,h,w] -> (z_q [B,C,h,w], commit_loss); the indices of the last call stay in ``self.indices``."""
        z_q, self.indices, commit_loss = self.vq.quantize_nchw(z)
        return z_q, commit_loss

    @torch.no_grad()
    def fit_codebooks(self, batches, epochs=1, reset=False):
        """Fit the quantiser's codebooks to this encoder's latents: per batch (a tensor, or a tuple whose first entry is one) a
        ``no_grad`` encode and then the quantiser's training call (``ResidualVQ`` above: k-means initialisation of levels that are not
        initialised, EMA update, dead-code expiry); nothing else of the model changes.  ``reset=True`` clears ``initted`` first, so a loaded
        checkpoint's codebooks are refitted from scratch.  ``batches`` is walked ``epochs`` times (pass a list or a loader, not a
        generator, for more than one).  Returns (losses [calls, levels], expired codes [calls, levels]) as device tensors and leaves the
        model in eval mode.  Each data-parallel rank fits its own shard: the statistics are not reduced across ranks."""
        if reset:
            for layer in self.vq.layers:
                layer._codebook.initted.fill_(False)
        losses, expired = [], []
        self.eval()
        self.vq.train()
        try:
            for _ in range(int(epochs)):
                for x in batches:
                    z = self.encode(x[0] if isinstance(x, (tuple, list)) else x)
                    losses.append(self.vq.quantize_nchw(z)[2][0])
                    expired.append(self.vq.last_expired)
        finally:
            self.eval()
        if not losses:
            raise ValueError("VQVAE.fit_codebooks: no batches")
        return torch.stack(losses), torch.stack(expired)

    @torch.no_grad()
    def calc_distance_stats(self, z, z_q):
        """codecs.py:527-536 (diagnostic)."""
        z_flat = z.reshape(-1, z.shape[1])
        distances = torch.norm(z_flat.unsqueeze(1) - self.vq.codebooks[0].to(z.device), dim=-1)
        return {'codebook_mean_dist': distances.mean().item(), 'codebook_max_dist': distances.max().item()}

    def forward(self, x, noise_strength=None, minval=0, get_stats=False):
        """codecs.py:545-574 in eval mode: encode -> quantize -> decode; returns (recon, commit_loss.mean()[, stats])."""
        if self.training:
            raise NotImplementedError("VQVAE.forward: training mode (codec training) is out of scope; call .eval()")
        z = self.encode(x)
        if noise_strength is None:
            noise_strength = 0.0
        if self.info is None:
            self.info = z.shape
        z_q, commit_loss = self.quantize(z)
        x_recon = self.decode(z_q, noise_strength=noise_strength)
        if get_stats:
            return x_recon, commit_loss.mean(), self.calc_distance_stats(z, z_q)
        return x_recon, commit_loss.mean()

    def _op_record(self, decode, i):
        k, m, f, bp, bf = C.c_char_p(), C.c_char_p(), C.c_double(), C.c_double(), C.c_double()
        B.check(B.lib().fc_vqvae_op_info(self._handle, int(decode), i, C.byref(k), C.byref(m), C.byref(f), C.byref(bp), C.byref(bf)))
        return k.value.decode(), m.value.decode(), f.value, bp.value, bf.value


def _read_weights(path: str) -> Dict[str, torch.Tensor]:
    path = os.path.expanduser(path)
    if os.path.isdir(path):
        for cand in ("diffusion_pytorch_model.safetensors", "diffusion_pytorch_model.bin", "vae.safetensors", "vae.pt"):
            if os.path.exists(os.path.join(path, cand)):
                path = os.path.join(path, cand)
                break
        else:
            raise FileNotFoundError(f"no SD-VAE weight file under {path}")
    if not os.path.exists(path):
        raise FileNotFoundError(f"SD-VAE weights not found: {path}")
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path)
    sd = torch.load(path, map_location="cpu", weights_only=False)
    return sd.get("state_dict", sd.get("model_state_dict", sd))


def setup_codec(config, device, no_natten=False, load_checkpoint=True, eval=True):
    """codecs.py:668-741 -- codec factory keyed on ``config.codec.choice``."""
    choice = config.codec.choice if 'choice' in config.codec else None
    if choice is None or choice == "noop":
        print("Using NoOpAE")
        codec = NoOpAE().eval().to(device)
    elif choice == "resize":
        print("Using SimpleResizeAE")
        codec = SimpleResizeAE(latent_shape=tuple(config.codec.get('latent_shape', (4, 16, 16)))).eval().to(device)
    elif choice == "sd":
        print("Loading SD VAE via SD_VAE_Wrapper")
        weights = config.codec.get('sd_vae_path') or os.environ.get("FLOCODER_SD_VAE_PATH")
        codec = SD_VAE_Wrapper(pretrained_model_name="stabilityai/sd-vae-ft-mse", weights=weights).eval().to(device)
        if 'image_size' in config and config.image_size % 8 != 0:
            print(f"Warning: SD VAE works best with image sizes divisible by 8. Current size: {config.image_size}")
    elif choice == "vqgan_plus":
        raise NotImplementedError("codec 'vqgan_plus' is codec-training territory and outside the flow hot path (SURVEY.md 2)")
    else:
        print("Loading VQVAE model")
        checkpoint = None
        if load_checkpoint:
            if 'vqgan_checkpoint' in config:
                path = config.vqgan_checkpoint
            elif 'codec' in config and 'checkpoint' in config.codec:
                path = config.codec.checkpoint
            else:
                raise ValueError("Could not find codec checkpoint path in config")
            if path.lower() != "sd" and not os.path.exists(path):
                raise FileNotFoundError(f"Codec checkpoint file {path} not found.")
            print(f"Loading codec checkpoint from {path}")
            try:
                checkpoint = torch.load(path, map_location=device, weights_only=True)
            except Exception:
                checkpoint = torch.load(path, map_location=device, weights_only=False)
        # A checkpoint trained WITH the natten package carries NATTENBlock weights ('...attn.qkv.weight', codecs.py:93-145).  Upstream
        # such a model silently loses its attention when the package is missing; here the blocks are native
        # (fc_vqvae_create_ex), so they are built whenever the checkpoint has them -- unless no_natten asks for upstream's fallback.
        natten_layout = 0
        if checkpoint is not None and any(k.endswith('.attn.qkv.weight') for k in checkpoint['model_state_dict']):
            if no_natten:
                print("Warning: the checkpoint holds NATTEN attention blocks and no_natten=True drops them (as upstream without the package)")
            else:
                natten_layout = int(ldcfg(config, 'natten_layout', 2, verbose=False) or 2)
                print(f"Codec checkpoint holds NATTEN blocks: building them natively (natten_layout={natten_layout}; 2 = what natten >= 0.20, "
                      "the reference's pinned minimum, computes from its call; set codec.natten_layout=1 for windows over image rows x columns)")
        codec = VQVAE(                                                    # codecs.py:707-718
            in_channels=ldcfg(config, 'in_channels', 3, verbose=False),
            hidden_channels=ldcfg(config, 'hidden_channels', 256, verbose=False),
            num_downsamples=ldcfg(config, 'num_downsamples', 3, verbose=False),
            internal_dim=ldcfg(config, 'internal_dim', 256, verbose=False),
            vq_embedding_dim=ldcfg(config, 'vq_embedding_dim', 4, verbose=False),
            codebook_levels=ldcfg(config, 'codebook_levels', 4, verbose=False),
            vq_num_embeddings=ldcfg(config, 'vq_num_embeddings', 512, verbose=False),
            commitment_weight=ldcfg(config, 'commitment_weight', 0.5, verbose=False),
            use_checkpoint=not config.get('no_grad_ckpt', False),
            no_natten=no_natten, natten_layout=natten_layout,
        ).to(device)
        if checkpoint is not None:
            codec.load_state_dict(checkpoint['model_state_dict'], strict=False)   # strict=False: vq.* training buffers may be absent
    if eval:
        codec = codec.eval()
    print("Codec model ready")
    return codec
