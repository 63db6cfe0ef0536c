"""CPU restatement of flocoder's VQVAE codec encode / decode path (codecs.py:150-574), NATTEN-less.

TEST INFRASTRUCTURE ONLY -- see ``oracle/__init__.py``.  Parity status: PINNED for ``encode`` and ``decode`` --
``tools/make_golden.py`` runs the reference's own ``VQVAE`` (with a stand-in for the absent ``vector_quantize_pytorch``
package, which neither method calls) on seeded weights and ``tests/test_oracle_golden.py`` holds this file to the result
(fixture g9).  ``quantize`` = ``vector_quantize_pytorch.ResidualVQ`` (``>=1.22.4``, pyproject.toml:41; call sites codecs.py:456-467,
504-521) is third-party and absent: ``residual_vq`` / ``quantize`` below restate its published INFERENCE behaviour -- PARITY
UNPINNED.  NATTEN is absent here, so in the pinned fixtures ``attention='natten'`` blocks have no attention (codecs.py:170-175,
SURVEY Q23); state dicts that DO carry ``attn.qkv`` weights run ``natten_block`` / ``na2d`` below -- a restatement of the package's
published neighbourhood-attention definition, PARITY UNPINNED;
eval mode: dropout is the identity and NoiseInjection is a no-op at noise_strength 0 (codecs.py:229-232).
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
import torch.nn.functional as F

Tensor = torch.Tensor
SD = Dict[str, Tensor]


def gn_groups(proposed: int, channels: int) -> int:
    """codecs.py:34-44."""
    if channels % proposed == 0:
        return proposed
    for c in range(proposed, channels):
        if channels % c == 0:
            return c
    return 1


def _conv(sd, n, x, padding=0, stride=1):
    return F.conv2d(x, sd[n + ".weight"], sd.get(n + ".bias"), stride=stride, padding=padding)


def _gn(sd, n, x, proposed, eps=1e-5):
    c = x.shape[1]
    return F.group_norm(x, gn_groups(proposed, c), sd[n + ".weight"], sd[n + ".bias"], eps=eps)


# AttnBlock in four steps, every tensor NCHW as the library's taps are read back: q / k / v [b, c, h, w]; the scores after the softmax
# p [b, n_keys, h, w] (channel j of pixel i: the weight query i gives key j); o = p v [b, c, h, w].
def attn_qkv(sd: SD, n: str, x: Tensor):
    t = F.group_norm(x, gn_groups(32, x.shape[1]), sd[n + ".norm.norm.weight"], sd[n + ".norm.norm.bias"], eps=1e-6)
    return _conv(sd, n + ".q", t), _conv(sd, n + ".k", t), _conv(sd, n + ".v", t)


def attn_probs(q: Tensor, k: Tensor) -> Tensor:
    b, c, h, w = q.shape
    a = torch.softmax(torch.bmm(q.reshape(b, c, h * w).permute(0, 2, 1), k.reshape(b, c, h * w)) * int(c) ** -0.5, dim=2)
    return a.permute(0, 2, 1).reshape(b, h * w, h, w)


def attn_apply(p: Tensor, v: Tensor) -> Tensor:
    b, c, h, w = v.shape
    return torch.bmm(v.reshape(b, c, h * w), p.reshape(b, h * w, h * w)).reshape(b, c, h, w)


def attn_block(sd: SD, n: str, x: Tensor, taps: Optional[dict] = None, tap: str = "") -> Tensor:
    """AttnBlock, codecs.py:53-89: GroupNorm(32, eps 1e-6), 1x1 q/k/v, softmax(q^T k c^-1/2) over keys, proj_out, residual.
    ``taps[tap + ".q"]`` ... ``".o"``: the four steps' tensors."""
    q, k, v = attn_qkv(sd, n, x)
    p = attn_probs(q, k)
    o = attn_apply(p, v)
    if taps is not None:
        taps.update({tap + ".q": q, tap + ".k": k, tap + ".v": v, tap + ".p": p, tap + ".o": o})
    return x + _conv(sd, n + ".proj_out", o)


def na2d(q: Tensor, k: Tensor, v: Tensor, kernel_size: int = 7, scale: float | None = None) -> Tensor:
    """2-D neighbourhood attention on [B, X, Y, heads, d] tensors: query (x, y) attends to the kernel_size^2 keys of the window whose
    start along each axis is clamp(pos - kernel_size // 2, 0, L - kernel_size) (it shifts inwards at the borders: never padded), with
    softmax(q . k * scale) and scale = d^-0.5 by default.  Restates the PUBLISHED definition of ``natten.functional.na2d`` (dilation 1,
    non-causal, no relative position bias; natten >= 0.20.1, pyproject.toml:40).  PARITY UNPINNED: the package is absent."""
    B, X, Y, H, D = q.shape
    if X < kernel_size or Y < kernel_size:
        raise ValueError("neighbourhood larger than the attended axes")
    scale = D ** -0.5 if scale is None else scale
    r = kernel_size // 2
    sx = (torch.arange(X) - r).clamp(0, X - kernel_size)
    sy = (torch.arange(Y) - r).clamp(0, Y - kernel_size)
    ix = sx[:, None] + torch.arange(kernel_size)[None, :]                   # [X, K]
    iy = sy[:, None] + torch.arange(kernel_size)[None, :]                   # [Y, K]
    kw = k[:, ix][:, :, :, iy]                                              # [B, X, K, Y, K, H, D]
    vw = v[:, ix][:, :, :, iy]
    kw = kw.permute(0, 1, 3, 5, 2, 4, 6).reshape(B, X, Y, H, kernel_size * kernel_size, D)
    vw = vw.permute(0, 1, 3, 5, 2, 4, 6).reshape(B, X, Y, H, kernel_size * kernel_size, D)
    a = torch.softmax(torch.einsum("bxyhd,bxyhwd->bxyhw", q, kw) * scale, dim=-1)
    return torch.einsum("bxyhw,bxyhwd->bxyhd", a, vw)


def natten_qkv(sd: SD, n: str, x: Tensor) -> Tensor:
    """GroupNorm(gn_groups(8, C)) -> qkv Linear (no bias), as [B, 3C, H, W] (channel = which * C + head * d + i)."""
    t = F.group_norm(x, gn_groups(8, x.shape[1]), sd[n + ".norm.weight"], sd[n + ".norm.bias"]).permute(0, 2, 3, 1)      # B H W C
    return F.linear(t, sd[n + ".qkv.weight"]).permute(0, 3, 1, 2)


def natten_att(qkv: Tensor, layout: int = 1, heads: int = 8, kernel_size: int = 7) -> Tensor:
    """The neighbourhood attention of NATTENBlock on its qkv tensor [B, 3C, H, W] -> [B, C, H, W] (before proj and gamma)."""
    B, C3, H, W = qkv.shape
    C = C3 // 3
    d = C // heads
    qkv = qkv.permute(0, 2, 3, 1).reshape(B, H, W, 3, heads, d).permute(3, 0, 4, 1, 2, 5)                       # 3 B heads H W d
    q, k, v = qkv[0], qkv[1], qkv[2]
    if layout == 1:
        o = na2d(q.permute(0, 2, 3, 1, 4), k.permute(0, 2, 3, 1, 4), v.permute(0, 2, 3, 1, 4), kernel_size).permute(0, 3, 1, 2, 4)
    else:
        o = na2d(q, k, v, kernel_size)                                                                          # dims taken as [B, X, Y, heads, d]
    return o.permute(0, 2, 3, 1, 4).reshape(B, H, W, C).permute(0, 3, 1, 2)                                    # codecs.py:137


def natten_block(sd: SD, n: str, x: Tensor, layout: int = 1, heads: int = 8, kernel_size: int = 7, taps: Optional[dict] = None,
                 tap: str = "") -> Tensor:
    """NATTENBlock._forward, codecs.py:116-140: GroupNorm(gn_groups(8, C)) -> qkv Linear (no bias) -> neighbourhood attention ->
    proj Linear (no bias) -> identity + gamma * (.).  The reference builds q / k / v as [B, heads, H, W, d] (codecs.py:122-124).
    ``layout`` 1 reads that as intended (7x7 windows over image rows x columns, per head); ``layout`` 2 is what a natten >= 0.20
    ``na2d`` -- which documents [B, X, Y, heads, d] -- computes from the very same tensors: windows over (head index, image row), the
    image column playing the part of the head.  Which one a trained checkpoint needs can only be settled against the package.
    ``taps[tap + ".qkv"]``; ``taps[tap + ".att"]`` = gamma * attention, as the library keeps it (proj is linear and has no bias)."""
    qkv = natten_qkv(sd, n, x)
    o = natten_att(qkv, layout, heads, kernel_size)
    if taps is not None:
        taps[tap + ".qkv"], taps[tap + ".att"] = qkv, o * sd[n + ".gamma"]
    o = F.linear(o.permute(0, 2, 3, 1), sd[n + ".proj.weight"]).permute(0, 3, 1, 2)
    return x + o * sd[n + ".gamma"]


def block_act(sd: SD, n: str, h1: Tensor) -> Tensor:
    return F.silu(_gn(sd, n + ".norm1", h1, 8))


def block_close(sd: SD, n: str, h2: Tensor, x: Tensor, res: Optional[Tensor] = None) -> Tensor:
    """silu(norm2(h2) + identity): identity = x, or downsample.1 of ``res`` (the downsample.0 convolution of x)."""
    if res is not None:
        x = _gn(sd, n + ".downsample.1", res, 8)
    return F.silu(_gn(sd, n + ".norm2", h2, 8) + x)


def res_block(sd: SD, n: str, x: Tensor, stride: int = 1, natten_layout: int = 1, taps: Optional[dict] = None) -> Tensor:
    """EncDecResidualBlock._forward, codecs.py:178-209 (eval): silu(norm1(conv1 x)) [-> attn] -> norm2(conv2 .) + identity -> silu.
    ``taps``: ``n.h1`` conv1, ``n.act`` its activation where an attention reads it, ``n.mid`` what conv2 reads, ``n.h2`` conv2,
    ``n.res`` the downsample.0 convolution, ``n`` the output."""
    h1 = _conv(sd, n + ".conv1", x, padding=1, stride=stride)
    out = block_act(sd, n, h1)
    if taps is not None:
        taps[n + ".h1"] = h1
        if (n + ".attn.q.weight") in sd or (n + ".attn.qkv.weight") in sd:
            taps[n + ".act"] = out
    if (n + ".attn.q.weight") in sd:                       # attention='full'
        out = attn_block(sd, n + ".attn", out, taps, n)
    elif (n + ".attn.qkv.weight") in sd:                   # attention='natten' with the package present (else: no attention at all)
        out = natten_block(sd, n + ".attn", out, natten_layout, taps=taps, tap=n)
    h2 = _conv(sd, n + ".conv2", out, padding=1)
    res = _conv(sd, n + ".downsample.0", x, stride=stride) if (n + ".downsample.0.weight") in sd else None
    y = block_close(sd, n, h2, x, res)
    if taps is not None:
        taps[n + ".mid"], taps[n + ".h2"], taps[n] = out, h2, y
        if res is not None:
            taps[n + ".res"] = res
    return y


def rope(x: Tensor, scale: float = math.log(10000.0)) -> Tensor:
    """SpatialNonLocalAttention._apply_rope, codecs.py:351-369, on [b, hw, c]."""
    b, hw, c = x.shape
    if c % 2 != 0:
        x = F.pad(x, (0, 1)); c = x.shape[-1]
    pos = torch.arange(hw).unsqueeze(1)
    inv_freq = torch.exp(-torch.arange(0, c // 2) * scale / (c // 2))
    pe = pos * inv_freq.unsqueeze(0)
    ps, pc = torch.sin(pe).to(x.dtype), torch.cos(pe).to(x.dtype)
    xe, xo = x[..., 0::2], x[..., 1::2]
    out = torch.empty_like(x)
    out[..., 0::2] = xe * pc - xo * ps
    out[..., 1::2] = xo * pc + xe * ps
    return out


def spatial_nonlocal_attention(sd: SD, n: str, x: Tensor) -> Tensor:
    """codecs.py:371-383."""
    b, c, h, w = x.shape
    q = rope(_conv(sd, n + ".q_proj", x).reshape(b, -1, h * w).permute(0, 2, 1))
    k = rope(_conv(sd, n + ".k_proj", x).reshape(b, -1, h * w).permute(0, 2, 1))
    v = _conv(sd, n + ".v_proj", x).reshape(b, c, h * w).permute(0, 2, 1)
    a = F.softmax(torch.bmm(q, k.transpose(1, 2)) * (q.size(-1) ** -0.5), dim=-1)
    o = torch.bmm(a, v).permute(0, 2, 1).reshape(b, c, h, w)
    return x + _conv(sd, n + ".out_proj", o)


def n_downsamples(sd: SD) -> int:
    blocks = sorted({int(k.split(".")[1]) for k in sd if k.startswith("encoder.") and ".conv1.weight" in k})
    return (len(blocks) - 1) // 2


def _tap(taps, name, value):
    if taps is not None:
        taps[name] = value
    return value


def encode(sd: SD, x: Tensor, natten_layout: int = 1, taps: Optional[dict] = None) -> Tensor:
    """VQVAE.encode = self.encoder(x), codecs.py:414-443,492-502: 2 residual blocks per downsample (the first with stride 2), one
    more to internal_dim, a 1x1 conv, then the compress stack conv1x1 -> GroupNorm -> SiLU -> conv3x3.  ``taps``: every block's
    tensors (res_block) and the three convolutions of the tail, by state_dict prefix."""
    nd = n_downsamples(sd)
    h = x
    for i in range(nd):
        h = res_block(sd, f"encoder.{2 * i}", h, stride=2, natten_layout=natten_layout, taps=taps)
        h = res_block(sd, f"encoder.{2 * i + 1}", h, natten_layout=natten_layout, taps=taps)
    h = res_block(sd, f"encoder.{2 * nd}", h, natten_layout=natten_layout, taps=taps)
    h = _tap(taps, f"encoder.{2 * nd + 1}", _conv(sd, f"encoder.{2 * nd + 1}", h))
    h = _tap(taps, f"encoder.{2 * nd + 2}", _conv(sd, f"encoder.{2 * nd + 2}", h))
    return _tap(taps, f"encoder.{2 * nd + 5}", compress_out(sd, nd, h))


def compress_out(sd: SD, nd: int, h: Tensor) -> Tensor:
    return _conv(sd, f"encoder.{2 * nd + 5}", F.silu(_gn(sd, f"encoder.{2 * nd + 3}", h, 2)), padding=1)


def expand_out(sd: SD, i: int, h: Tensor, emb: int) -> Tensor:
    """decoder.layers.{i+1 .. i+3}: GroupNorm(gn_groups(emb, C)) -> SiLU -> conv1x1."""
    return _conv(sd, f"decoder.layers.{i + 3}", F.silu(_gn(sd, f"decoder.layers.{i + 1}", h, emb)))


def decode(sd: SD, z: Tensor, natten_layout: int = 1, taps: Optional[dict] = None) -> Tensor:
    """VQVAE.decode -> Decoder.forward at noise_strength 0, codecs.py:245-316,523-525.  ``taps``: by ``decoder.layers.<index>``; a
    convolution followed by SiLU is recorded after the SiLU, the PixelShuffle under its own index."""
    nd = n_downsamples(sd)
    L = "decoder.layers."
    i = 0
    h = z
    if (L + "0.q_proj.weight") in sd:
        h = _tap(taps, L + "0", spatial_nonlocal_attention(sd, L + "0", h)); i = 1
    h = _tap(taps, L + str(i), _conv(sd, L + str(i), h))
    h = _tap(taps, L + str(i + 3), expand_out(sd, i, h, z.shape[1]))
    h = res_block(sd, L + str(i + 5), h, natten_layout=natten_layout, taps=taps)   # i+4 is a NoiseInjection
    i += 6
    for _ in range(nd):
        h = _tap(taps, L + str(i), F.silu(_conv(sd, L + str(i), h, padding=1)))     # conv, SiLU, PixelShuffle(2), NoiseInjection
        h = _tap(taps, L + str(i + 2), F.pixel_shuffle(h, 2))
        h = res_block(sd, L + str(i + 4), h, natten_layout=natten_layout, taps=taps)
        h = res_block(sd, L + str(i + 6), h, taps=taps)                              # i+5 is a NoiseInjection
        i += 7
    h = _tap(taps, L + str(i + 1), F.silu(_conv(sd, L + str(i + 1), h, padding=1)))   # i is a NoiseInjection
    return _tap(taps, L + str(i + 4), _conv(sd, L + str(i + 4), h, padding=1))        # i+2 SiLU, i+3 NoiseInjection


def residual_vq(codebooks: Tensor, x: Tensor):
    """ResidualVQ.forward in eval mode on flattened vectors x [N, D] with codebooks [L, K, D] (vector_quantize_pytorch: per layer
    ``embed_ind = argmax(-cdist(residual, embed))``, ``quantize = embed[embed_ind]``, ``residual -= quantize``; outputs the sum of the
    layers' codewords, indices [N, L] and -- nothing is learnt in eval -- zero losses [1, L]).  PARITY UNPINNED (third party)."""
    residual, out, idx = x.clone(), torch.zeros_like(x), []
    for cb in codebooks:
        d = ((residual[:, None, :] - cb[None, :, :]) ** 2).sum(-1)
        i = d.argmin(dim=1)
        q = cb[i]
        residual = residual - q
        out = out + q
        idx.append(i)
    return out, torch.stack(idx, dim=-1), torch.zeros(1, codebooks.shape[0])


def quantize(sd: SD, z: Tensor):
    """VQVAE.quantize, codecs.py:504-521: permute to [N, C], ResidualVQ, back to NCHW.  Codebooks = ``vq.layers.{i}._codebook.embed``
    ([1, K, D] each).  Returns (z_q, commit_loss [1, L], indices [N, L])."""
    L = len({k.split(".")[2] for k in sd if k.startswith("vq.layers.") and k.endswith("._codebook.embed")})
    cbs = torch.stack([sd[f"vq.layers.{i}._codebook.embed"].reshape(-1, z.shape[1]) for i in range(L)])
    zp = z.permute(0, 2, 3, 1)
    zq, idx, loss = residual_vq(cbs, zp.reshape(-1, z.shape[1]))
    return zq.view(zp.shape).permute(0, 3, 1, 2).contiguous(), loss, idx
