"""The counter-based normal field of the stochastic samplers, on the host (NumPy): what ``fc_ode_normal_field`` and the update kernel of
``fc_unet_integrate_sde`` generate on the device (csrc/ode.hip), value for value up to the fp32 rounding of the device's functions.

A value is indexed by what it is, never by where it sits in a launch or a batch:

    key     = (seed & 0xffffffff, seed >> 32)
    counter = (j, draw_index, sample_id & 0xffffffff, sample_id >> 32)

with ``j`` the index of the group of four inside the sample's ``per_sample`` elements and ``draw_index`` the interval of the sampler's grid,
counted from the call's first interval.  Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; multipliers
0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85) turns the pair into four words ``r0..r3``; the uniforms
``u_k = ((r_k >> 9) + 0.5) 2^-23`` are exact in fp32 and lie in ``[2^-24, 1 - 2^-24]``; elements ``4j .. 4j+3`` are

    sqrt(-2 ln u0) cos(2 pi u1),  sqrt(-2 ln u0) sin(2 pi u1),  sqrt(-2 ln u2) cos(2 pi u3),  sqrt(-2 ln u2) sin(2 pi u3)

so the tail is cut at ``|z| <= sqrt(-2 ln 2^-24) = sqrt(48 ln 2) = 5.77`` (probability 8e-9 per value beyond it for a true normal).  Here
the transform runs in fp64 on the exact uniforms; the device evaluates it in fp32 (DESIGN.md section 4b has the operation sequence).
"""
from __future__ import annotations

import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xffffffff)
_S32 = np.uint64(32)
TAIL = float(np.sqrt(48 * np.log(2.0)))


def philox4x32(counter, key, rounds: int = 10) -> np.ndarray:
    """Philox4x32 block function, vectorised: ``counter`` ``[..., 4]`` and ``key`` ``[..., 2]`` (broadcast against each other) of 32-bit
    words -> ``[..., 4]`` uint32."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK
    k = np.asarray(key, dtype=np.uint64) & _MASK
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape) for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape) for i in range(2))
    for r in range(rounds):
        p0, p1 = _M0 * c0, _M1 * c2                       # 32 x 32 -> 64 bit products, exact in uint64
        kr0 = (k0 + np.uint64((_W0 * r) & 0xffffffff)) & _MASK
        kr1 = (k1 + np.uint64((_W1 * r) & 0xffffffff)) & _MASK
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ kr0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ kr1, p0 & _MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def field_words(seed: int, draw_index: int, sample_ids, per_sample: int) -> np.ndarray:
    """The Philox output words of the field: uint32 ``[B, per_sample // 4, 4]``."""
    per_sample = int(per_sample)
    if per_sample < 4 or per_sample % 4:
        raise ValueError(f"per_sample={per_sample} must be a positive multiple of 4 (one Philox block per four values)")
    if not 0 <= int(draw_index) <= 0xffffffff:
        raise ValueError("draw_index is a 32-bit counter word")
    seed = int(seed) & 0xffffffffffffffff
    sid = np.asarray(sample_ids, dtype=np.int64).reshape(-1).astype(np.uint64)      # two's complement, as the device reads an int64
    groups = per_sample // 4
    ctr = np.empty((sid.size, groups, 4), dtype=np.uint64)
    ctr[..., 0] = np.arange(groups, dtype=np.uint64)[None, :]
    ctr[..., 1] = np.uint64(int(draw_index))
    ctr[..., 2] = (sid & _MASK)[:, None]
    ctr[..., 3] = (sid >> _S32)[:, None]
    return philox4x32(ctr, np.array([seed & 0xffffffff, seed >> 32], dtype=np.uint64))


def uniforms(words: np.ndarray) -> np.ndarray:
    """``((r >> 9) + 0.5) 2^-23`` as fp64 (every value is an fp32 number)."""
    return ((words >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def normal_field(seed: int, draw_index: int, sample_ids, per_sample: int) -> np.ndarray:
    """fp64 ``[B, per_sample]``: row b holds the normals of ``(seed, draw_index, sample_ids[b])``."""
    u = uniforms(field_words(seed, draw_index, sample_ids, per_sample))
    r0, r1 = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
    a0, a1 = 2.0 * np.pi * u[..., 1], 2.0 * np.pi * u[..., 3]
    z = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=-1)
    return z.reshape(z.shape[0], int(per_sample))


# ---- the likelihood's probe field (csrc/ode.hip, fc_ode_probe_field) ----------------------------------------------------------------------
PROBE_KEY_OFFSET = 0x50524F4245464C44      # "PROBEFLD": added to the seed (mod 2^64), so a likelihood seed does not replay the SDE noise
PROBE_KINDS = {"rademacher": 0, "gaussian": 1}


def probe_field(seed: int, probe_index: int, sample_ids, per_sample: int, kind="rademacher") -> np.ndarray:
    """fp32 ``[B, per_sample]``: row b holds Hutchinson probe ``probe_index`` of ``(seed, sample_ids[b])``, what ``fc_ode_probe_field``
    writes.  The Philox key is ``seed + PROBE_KEY_OFFSET`` (mod 2^64), the counter ``(j, probe_index, sample id lo, sample id hi)`` with
    ``j`` the group of four inside the sample: an entry depends on (seed, probe index, sample id, position) and on nothing else.
    ``"rademacher"`` (or 0): +1 where the top bit of the entry's Philox word is clear, -1 where it is set -- the device's bits exactly.
    ``"gaussian"`` (or 1): ``normal_field``'s uniforms and transform under that key (tail cut at 5.77), evaluated in fp64 and rounded once
    to fp32 -- the device does the same (fp64 transform, one rounding), so the two agree in bits."""
    kind = PROBE_KINDS.get(kind, kind)
    if kind not in (0, 1):
        raise ValueError(f"kind={kind!r}: 'rademacher' (0) or 'gaussian' (1)")
    key = (int(seed) + PROBE_KEY_OFFSET) & 0xffffffffffffffff
    if kind == 1:
        return normal_field(key, probe_index, sample_ids, per_sample).astype(np.float32)
    w = field_words(key, probe_index, sample_ids, per_sample)
    return (1.0 - 2.0 * (w >> np.uint32(31)).astype(np.float32)).reshape(w.shape[0], int(per_sample))


# ---- the plan sampler's uniforms (csrc/ot_plan.hip, fc_ot_sample_plan) ------------------------------------------------------------------
PLAN_TAG = 0x4F54504C            # "OTPL": counter word 2 of the plan sampler; word 3 is 0xFFFFFFFF, a sample id no non-negative int64 has


def uniforms53(r0, r1) -> np.ndarray:
    """``((r0 >> 5) 2^26 + (r1 >> 6) + 0.5) 2^-53`` as fp64: a 53-bit uniform from two Philox words, in (0, 1) -- but for the single
    pair of words with all 53 bits set, whose sum 2^53 - 1/2 rounds to 2^53 (u = 1); inversion clamps to the last cell."""
    hi = (np.asarray(r0, dtype=np.uint32) >> np.uint32(5)).astype(np.float64)
    lo = (np.asarray(r1, dtype=np.uint32) >> np.uint32(6)).astype(np.float64)
    return (hi * 67108864.0 + lo + 0.5) * 2.0 ** -53


def plan_uniforms(seed: int, draw_index: int, n: int) -> np.ndarray:
    """fp64 ``[n]``: the uniform that ``fc_ot_sample_plan`` inverts for pair k of draw ``draw_index``: words 0 and 1 of the Philox block
    with counter ``(k, draw_index, PLAN_TAG, 0xFFFFFFFF)`` and the seed's two words as the key."""
    if not 0 <= int(draw_index) <= 0xffffffff:
        raise ValueError("draw_index is a 32-bit counter word")
    if not 0 <= int(n) <= 0xffffffff:
        raise ValueError("n must fit a 32-bit counter word")
    seed = int(seed) & 0xffffffffffffffff
    ctr = np.empty((int(n), 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(int(n), dtype=np.uint64)
    ctr[:, 1] = np.uint64(int(draw_index))
    ctr[:, 2] = np.uint64(PLAN_TAG)
    ctr[:, 3] = np.uint64(0xFFFFFFFF)
    w = philox4x32(ctr, np.array([seed & 0xffffffff, seed >> 32], dtype=np.uint64))
    return uniforms53(w[:, 0], w[:, 1])


# ---- the inpainting mask field (csrc/masks.hip, fc_inpaint_masks) -------------------------------------------------------------------------
# A counter-based restatement of upstream's generate_mask (flocoder/inpainting.py:277-351): a mask is a function of (seed, sample id, H, W,
# type probabilities | forced type) and of nothing else.  Key = seed + MASK_KEY_OFFSET (mod 2^64); counter = (j, region, sample id lo,
# sample id hi), where ``region`` says what the block is for:
#
#   region 0, j = 0          word 0: the type (against the cumulative p, as 32-bit thresholds floor(cum 2^32)); word 1: the number of
#                            brush strokes, 2 + mulhi(w, 4); word 2: the number of rectangles, 2 + mulhi(w, 9)
#   region 1, j              'noise': pixels 4j .. 4j+3 of the flattened [H, W] image, set where (w >> 9) >= 5872026, i.e. where the
#                            field's uniform ((w >> 9) + 0.5) 2^-23 exceeds 0.7
#   region 2, j = rectangle  words 0..3: w, h, x, y of generate_rectangles, in that order
#   region 3 + s, j = 0      stroke s: words 0..3: bs, start x, start y, length;  j = 1: word 0: the start direction
#   region 3 + s, j = 2 + t  step t of stroke s: the direction kick sum_k mulhi(w_k, 723) - 1444 over the four words, and the radius
#                            offset from the low half of word 3, ((w_3 & 0xffff) * bs) >> 16
#
# ``randint(lo, hi)`` is ``lo + mulhi(w, hi - lo)`` (the high word of the 64-bit product): every draw is an integer and the two sides share
# every bit.  The brush walk is in integers too, because cosf / logf differ between a GPU and libm and a float walk would put some disc
# centres on different pixels: the direction is a binary angle (units of 2 pi / 65536, kept mod 2^16), the kick an integer sum of four
# uniforms on [0, 723) minus 1444 (std 417.4 units = 0.0400 rad: upstream's normal(0, 0.04), as an Irwin-Hall sum), the step comes from
# the committed table csrc/mask_trig.h -- MASK_TRIG[a] = rint(0.7 * 65536 * cos(2 pi a / 4096)), the sine is the entry a quarter turn back
# -- which this module parses and masks.hip includes, so neither side evaluates a cosine; the position is Q16 and the pixel is ``>> 16``.
MASK_KEY_OFFSET = 0x4D41534B464C4431       # "MASKFLD1"
MASK_TYPES = ("total", "brush", "rectangles", "noise", "nothing")      # the codes 0..4 of fc_inpaint_masks
MASK_DEFAULT_P = (0.4, 0.35, 0.15, 0.05, 0.05)
MASK_MIN_SIZE, MASK_MAX_SIZE = 16, 1024
MASK_MAX_CHOICES = 16
MASK_MAX_STROKES, MASK_MAX_STEPS, MASK_MAX_RECTS, MASK_MAX_RADIUS = 5, 300, 10, 20
MASK_TRIG_BITS = 12
MASK_NOISE_THRESHOLD = 5872026             # ceil(0.7 * 2^23 - 0.5)
_MASK_TRIG = None


def mask_trig_table() -> np.ndarray:
    """int64 [4096]: the numbers of csrc/mask_trig.h, read from that file (the device compiles the same file in)."""
    global _MASK_TRIG
    if _MASK_TRIG is None:
        import os
        import re
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "mask_trig.h")) as f:
            body = f.read()
        body = body[body.index("{", body.index("MASK_TRIG[")) + 1:body.rindex("}")]
        tab = np.array([int(v) for v in re.findall(r"-?\d+", body)], dtype=np.int64)
        if tab.size != 1 << MASK_TRIG_BITS:
            raise RuntimeError(f"csrc/mask_trig.h holds {tab.size} entries, not {1 << MASK_TRIG_BITS}")
        _MASK_TRIG = tab
    return _MASK_TRIG


def mask_trig_formula() -> np.ndarray:
    """What the committed table is defined as: ``rint(0.7 * 65536 * cos(2 pi a / 4096))``, one rounding of the fp64 value."""
    a = np.arange(1 << MASK_TRIG_BITS, dtype=np.float64)
    return np.rint(np.cos(a * (2.0 * np.pi / (1 << MASK_TRIG_BITS))) * (0.7 * 65536.0)).astype(np.int64)


def mask_type_thresholds(choices=MASK_TYPES, p=MASK_DEFAULT_P):
    """(codes int32 [n], thresholds uint64 [n]): type k is chosen where the type word is below ``thresholds[k]`` and not below
    ``thresholds[k-1]``; ``thresholds[k] = floor(cum_k 2^32)`` with the cumulative sum taken left to right in fp64, and the last one is
    2^32.  The library forms the same numbers the same way."""
    choices, p = list(choices), [float(v) for v in p]
    if not 1 <= len(choices) <= MASK_MAX_CHOICES or len(p) != len(choices):
        raise ValueError(f"choices and p must have the same length, 1 to {MASK_MAX_CHOICES}")
    for c in choices:
        if c not in MASK_TYPES:
            raise ValueError(f"Unsupported mask_type: {c}")
    if any(not 0.0 <= v <= 1.0 for v in p) or abs(sum(p) - 1.0) > 1e-8:
        raise ValueError("p must be probabilities that sum to 1")
    thr, cum = [], 0.0
    for v in p:
        cum += v
        thr.append(min(int(np.floor(cum * 4294967296.0)), 1 << 32))
    thr[-1] = 1 << 32
    return np.array([MASK_TYPES.index(c) for c in choices], dtype=np.int32), np.array(thr, dtype=np.uint64)


def _mask_key(seed: int) -> np.ndarray:
    key = (int(seed) + MASK_KEY_OFFSET) & 0xffffffffffffffff
    return np.array([key & 0xffffffff, key >> 32], dtype=np.uint64)


def mask_words(seed: int, sample_ids, region, j) -> np.ndarray:
    """uint64 ``[B, *j.shape, 4]`` (32-bit values): the Philox blocks with counter ``(j, region, sample id)`` under the mask key;
    ``region`` and ``j`` broadcast against each other."""
    sid = np.asarray(sample_ids, dtype=np.int64).reshape(-1).astype(np.uint64)
    j, region = np.broadcast_arrays(np.asarray(j, dtype=np.uint64), np.asarray(region, dtype=np.uint64))
    ex = (slice(None),) + (None,) * j.ndim
    ctr = np.empty((sid.size, *j.shape, 4), dtype=np.uint64)
    ctr[..., 0] = j[None]
    ctr[..., 1] = region[None]
    ctr[..., 2] = (sid & _MASK)[ex]
    ctr[..., 3] = (sid >> _S32)[ex]
    return philox4x32(ctr, _mask_key(seed)).astype(np.uint64)


def _mulhi(w, n):
    return ((w * np.uint64(n)) >> _S32).astype(np.int64)


def _check_mask_size(size):
    h, w = (int(v) for v in size)
    if not (MASK_MIN_SIZE <= h <= MASK_MAX_SIZE and MASK_MIN_SIZE <= w <= MASK_MAX_SIZE):
        raise ValueError(f"mask size {h}x{w}: both sides must lie in [{MASK_MIN_SIZE}, {MASK_MAX_SIZE}]")
    return h, w


def mask_types(seed: int, sample_ids, choices=MASK_TYPES, p=MASK_DEFAULT_P, mask_type="") -> np.ndarray:
    """int32 [B]: the type code (index into ``MASK_TYPES``) of every sample id; ``mask_type`` forces one."""
    sid = np.asarray(sample_ids, dtype=np.int64).reshape(-1)
    if mask_type != "":
        if mask_type not in MASK_TYPES:
            raise ValueError(f"Unsupported mask_type: {mask_type}")
        return np.full(sid.size, MASK_TYPES.index(mask_type), dtype=np.int32)
    codes, thr = mask_type_thresholds(choices, p)
    w0 = mask_words(seed, sid, 0, 0)[:, 0]
    return codes[np.searchsorted(thr, w0, side="right")]


def _half_widths() -> np.ndarray:
    """[cb, |dy|] -> the largest h >= 0 with h^2 + dy^2 <= cb^2 (-1 where |dy| > cb): the disc's half width on a row, in integers."""
    r = MASK_MAX_RADIUS
    cb, dy, h = np.arange(r + 1)[:, None, None], np.arange(r + 1)[None, :, None], np.arange(r + 1)[None, None, :]
    return np.where(h * h + dy * dy <= cb * cb, h, -1).max(axis=2)


def _brush(seed, sid, h, w):
    """The brush masks of the sample ids ``sid``: bool [B, h, w]."""
    nb = sid.size
    tab = mask_trig_table()
    tmask = (1 << MASK_TRIG_BITS) - 1
    n_strokes = 2 + _mulhi(mask_words(seed, sid, 0, 0)[:, 1], 4)                                   # [B]: 2..5
    regions = 3 + np.arange(MASK_MAX_STROKES)
    hd = mask_words(seed, sid, regions, 0)                                                          # [B, S, 4]
    bs = 3 + _mulhi(hd[..., 0], 12)                                                                 # randint(3, 15)
    x0 = _mulhi(hd[..., 1], w)                                                                      # randint(0, W): the column
    y0 = h // 3 + _mulhi(hd[..., 2], 2 * h // 3 - h // 3)                                           # randint(H//3, 2H//3): the row
    length = 100 + _mulhi(hd[..., 3], 200)                                                          # randint(100, 300)
    d0 = _mulhi(mask_words(seed, sid, regions, 1)[..., 0], 2 * 3277 + 1) - 3277                     # +- pi/10 = 3277 units
    d0 = d0 + np.where(2 * x0 > w, 32768, 0)
    st = mask_words(seed, sid, regions[:, None], 2 + np.arange(MASK_MAX_STEPS)[None, :])            # [B, S, T, 4]
    kick = _mulhi(st[..., 0], 723) + _mulhi(st[..., 1], 723) + _mulhi(st[..., 2], 723) + _mulhi(st[..., 3], 723) - 1444
    d = (d0[..., None] + np.cumsum(kick, axis=-1)) & 0xffff
    a = d >> (16 - MASK_TRIG_BITS)
    px = (x0[..., None] << 16) + np.cumsum(tab[a], axis=-1)                                         # Q16, after the step
    py = (y0[..., None] << 16) + np.cumsum(tab[(a - (1 << (MASK_TRIG_BITS - 2))) & tmask], axis=-1)
    out = (px < 0) | (px >= (w << 16)) | (py < 0) | (py >= (h << 16))
    t = np.arange(MASK_MAX_STEPS)
    alive = (np.cumsum(out, axis=-1) == 0) & (t < length[..., None]) & (np.arange(MASK_MAX_STROKES)[None, :, None] < n_strokes[:, None, None])
    roff = ((st[..., 3] & np.uint64(0xffff)) * bs[..., None].astype(np.uint64) >> np.uint64(16)).astype(np.int64)
    cb = np.maximum(1, bs[..., None] - ((bs[..., None] + 1) >> 1) + roff)                           # bs + randint(-bs//2, bs//2), floor division
    b_i, s_i, t_i = np.nonzero(alive)
    xi, yi, cb = px[b_i, s_i, t_i] >> 16, py[b_i, s_i, t_i] >> 16, cb[b_i, s_i, t_i]
    hw_tab = _half_widths()
    pitch = w + 1
    starts, stops = [], []
    for dy in range(-MASK_MAX_RADIUS, MASK_MAX_RADIUS + 1):                                         # spans of the discs, one row offset at a time
        row = yi + dy
        sel = (abs(dy) <= cb) & (row >= 0) & (row < h)
        hw = hw_tab[cb[sel], abs(dy)]
        base = (b_i[sel] * h + row[sel]) * pitch
        lo, hi = np.maximum(xi[sel] - hw, 0), np.minimum(xi[sel] + hw, w - 1) + 1
        ok = lo < hi
        starts.append(base[ok] + lo[ok])
        stops.append(base[ok] + hi[ok])
    n = nb * h * pitch
    diff = np.bincount(np.concatenate(starts), minlength=n) - np.bincount(np.concatenate(stops), minlength=n)
    return np.cumsum(diff.reshape(nb, h, pitch), axis=-1)[..., :w] > 0


def _rectangles(seed, sid, h, w):
    n = 2 + _mulhi(mask_words(seed, sid, 0, 0)[:, 2], 9)                                            # randint(2, 11)
    r = mask_words(seed, sid, 2, np.arange(MASK_MAX_RECTS))                                         # [B, R, 4]
    rw = 3 + _mulhi(r[..., 0], (w * 4) // 5 - 3)                                                    # randint(3, int(0.8 W))
    rh = 3 + _mulhi(r[..., 1], (h * 3) // 10 - 3)                                                   # randint(3, int(0.3 H))
    rx = _mulhi(r[..., 2], w - rw)                                                                  # randint(0, W - w)
    ry = _mulhi(r[..., 3], h - rh)                                                                  # randint(0, H - h)
    live = np.arange(MASK_MAX_RECTS)[None, :] < n[:, None]
    yy, xx = np.arange(h)[None, None, :, None], np.arange(w)[None, None, None, :]
    e = lambda v: v[:, :, None, None]
    inside = (xx >= e(rx)) & (xx < e(rx + rw)) & (yy >= e(ry)) & (yy < e(ry + rh)) & e(live)
    return inside.any(axis=1)


def _noise(seed, sid, h, w):
    groups = (h * w + 3) // 4
    wd = mask_words(seed, sid, 1, np.arange(groups)).reshape(sid.size, groups * 4)[:, :h * w]
    return ((wd >> np.uint64(9)) >= MASK_NOISE_THRESHOLD).reshape(sid.size, h, w)


def mask_field(seed: int, sample_ids, size=(128, 128), choices=MASK_TYPES, p=MASK_DEFAULT_P, mask_type="", return_types=False):
    """fp32 0/1 ``[B, 1, H, W]``: the inpainting mask of every ``(seed, sample_ids[b])`` at ``size = (H, W)``, what ``fc_inpaint_masks``
    writes, bit for bit (with ``return_types`` also the int32 ``[B]`` type codes, indices into ``MASK_TYPES``).  A counter-based
    restatement of upstream's ``generate_mask``: the type from one uniform against the cumulative ``p`` of ``choices`` (or forced by
    ``mask_type``); 'total' all ones, 'nothing' all zeros, 'noise' a per-pixel uniform > 0.7, 'rectangles' upstream's
    ``generate_rectangles`` draw for draw, 'brush' its ``simulate_brush_stroke`` with 2-5 strokes and an integer walk (the comment above
    has the counter layout and the walk).

    Non-square sizes.  Upstream mixes its two axes (it draws x against ``size[0]`` and then uses it as a column, bounds rows by
    ``size[0]`` and columns by ``size[1]``, and returns the transposed shape for rectangles), which only a square size hides.  This
    function defines the convention of this package: the mask is ``[H, W]``, ``x`` is a column in ``[0, W)`` and ``y`` a row in
    ``[0, H)`` everywhere -- the brush starts at a column drawn from ``[0, W)`` and a row from the middle third ``[H//3, 2H//3)``, turns
    round where ``2x > W`` and stops where it leaves ``[0, W) x [0, H)``; a rectangle is up to ``int(0.8 W)`` wide and ``int(0.3 H)``
    high (``4W // 5`` and ``3H // 10``).  At a square size that is upstream's distribution."""
    h, w = _check_mask_size(size)
    sid = np.asarray(sample_ids, dtype=np.int64).reshape(-1)
    types = mask_types(seed, sid, choices, p, mask_type)
    out = np.zeros((sid.size, 1, h, w), dtype=np.float32)
    out[types == 0] = 1.0
    for code, fn in ((1, _brush), (2, _rectangles), (3, _noise)):
        rows = np.nonzero(types == code)[0]
        for lo in range(0, rows.size, 256):                                                        # bounded working set
            sel = rows[lo:lo + 256]
            out[sel, 0] = fn(seed, sid[sel], h, w)
    return (out, types) if return_types else out
