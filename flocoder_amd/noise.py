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


# ---- pre-encoding augmentation (csrc/augment.hip, fc_augment_images / fc_augment_midi) -------------------------------------------------
# A counter-based restatement of upstream's two pipelines (flocoder/data.py:49-111).  Key = seed + AUG_KEY_OFFSET (mod 2^64); counter =
# (j, region, sample id lo, sample id hi):
#
#   region 0, j = 0          image_transforms: words 0, 1: the angle (a 53-bit uniform on [-15, 15] degrees); word 2: flip where its top bit
#                            is clear
#   region 0, j = 1 + t      try t < 10 of RandomResizedCrop: word 0: the area fraction, word 1: the log-ratio (uniforms (w + 1/2) 2^-32),
#                            words 2, 3: the box's top and left, mulhi(w, positions that fit)
#   region 1, j = 0          midi_transforms: word 0: RandomRoll fires where its top bit is clear; words 1, 2: the horizontal and vertical shift
#   region 1, j = 1          RandomCrop: words 0, 1: top and left
#
# The draws are made HERE, on the host, for the device too: the kernels receive one row of integers per sample (``augment_image_table`` /
# ``augment_midi_table``), so which source pixel a tap reads is the same integer decision on both sides.
AUG_KEY_OFFSET = 0x415547464C443031        # "AUGFLD01"
AUG_MIN_SIZE, AUG_MAX_SIZE, AUG_MAX_SIDE = 16, 1024, 8192
AUG_IMAGE_WORDS, AUG_MIDI_WORDS = 16, 8
AUG_TILE, AUG_LDS_PIXELS = 16, 6144          # fc_augment_images: the output tile of a workgroup; the largest window of the crop it stages in LDS
AUG_TRIES = 10
AUG_DEGREES, AUG_SCALE, AUG_RATIO, AUG_CENTER = 15.0, (0.8, 1.0), (3.0 / 4.0, 4.0 / 3.0), 0.9
AUG_MAX_V_SHIFT = 24


def aug_words(seed: int, sample_ids, region, j) -> np.ndarray:
    """uint64 ``[B, *j.shape, 4]`` (32-bit values): the Philox blocks with counter ``(j, region, sample id)`` under the augmentation key."""
    key = (int(seed) + AUG_KEY_OFFSET) & 0xffffffffffffffff
    sid = np.asarray(sample_ids, dtype=np.int64).reshape(-1).astype(np.uint64)
    j, region = np.broadcast_arrays(np.asarray(j, dtype=np.uint64), np.asarray(region, dtype=np.uint64))
    ex = (slice(None),) + (None,) * j.ndim
    ctr = np.empty((sid.size, *j.shape, 4), dtype=np.uint64)
    ctr[..., 0] = j[None]
    ctr[..., 1] = region[None]
    ctr[..., 2] = (sid & _MASK)[ex]
    ctr[..., 3] = (sid >> _S32)[ex]
    return philox4x32(ctr, np.array([key & 0xffffffff, key >> 32], dtype=np.uint64)).astype(np.uint64)


def _u32(w) -> np.ndarray:
    return (w.astype(np.float64) + 0.5) * 2.0 ** -32


def _check_aug_size(image_size) -> int:
    s = int(image_size)
    if not AUG_MIN_SIZE <= s <= AUG_MAX_SIZE:
        raise ValueError(f"image_size={s} must lie in [{AUG_MIN_SIZE}, {AUG_MAX_SIZE}]")
    return s


def _src_hw(src_hw, n) -> np.ndarray:
    hw = np.broadcast_to(np.asarray(src_hw, dtype=np.int64).reshape(-1, 2), (n, 2))
    if hw.size and (hw.min() < 2 or hw.max() > AUG_MAX_SIDE):
        raise ValueError(f"source sides must lie in [2, {AUG_MAX_SIDE}]")
    return hw


def augment_image_params(seed: int, sample_ids, src_hw, image_size) -> dict:
    """The draws of upstream's ``image_transforms`` for every ``(seed, sample_ids[b])`` on a source of ``src_hw`` (one ``(H, W)`` or one
    per sample), as a dict of ``[B]`` arrays.  ``angle`` (fp64 degrees, uniform on [-15, 15], counter-clockwise as PIL's).  The centre crop
    is deterministic: ``crop_side = int(0.9 min(H, W))`` at ``crop_top = round((H - side) / 2)``, ``crop_left`` likewise (round half to
    even, CenterCrop's).  ``RandomResizedCrop(scale=(0.8, 1), ratio=(3/4, 4/3))`` on that square: ten tries from fixed counters, try t
    draws ``area = side^2 (0.8 + 0.2 u)``, ``ratio = exp(uniform(log 3/4, log 4/3))``, ``w = round(sqrt(area ratio))``, ``h =
    round(sqrt(area / ratio))`` and is accepted where ``0 < w <= side`` and ``0 < h <= side``; its ``box_top`` / ``box_left`` are
    uniform integers over the positions that fit.  The first accepted try is taken (``tries`` is its index, ``area_frac`` and ``ratio``
    its draws); after ten failures (``tries = 10``, NaN draws) the box is upstream's fallback, the central box with the ratio clamped to
    [3/4, 4/3] -- the whole crop, a square's ratio being 1.  ``flip`` with p = 0.5.  The box is in the centre crop's coordinates."""
    _check_aug_size(image_size)
    sid = np.asarray(sample_ids, dtype=np.int64).reshape(-1)
    hw = _src_hw(src_hw, sid.size)
    h_src, w_src = hw[:, 0], hw[:, 1]
    head = aug_words(seed, sid, 0, 0)
    angle = -AUG_DEGREES + 2.0 * AUG_DEGREES * uniforms53(head[:, 0].astype(np.uint32), head[:, 1].astype(np.uint32))
    flip = (head[:, 2] >> np.uint64(31)) == 0
    side = (np.minimum(h_src, w_src) * AUG_CENTER).astype(np.int64)
    top = np.rint((h_src - side) / 2.0).astype(np.int64)
    left = np.rint((w_src - side) / 2.0).astype(np.int64)
    tr = aug_words(seed, sid, 0, 1 + np.arange(AUG_TRIES))                                          # [B, 10, 4]
    frac = AUG_SCALE[0] + (AUG_SCALE[1] - AUG_SCALE[0]) * _u32(tr[..., 0])
    lo, hi = np.log(AUG_RATIO[0]), np.log(AUG_RATIO[1])
    ratio = np.exp(lo + (hi - lo) * _u32(tr[..., 1]))
    area = (side * side)[:, None] * frac
    bw = np.rint(np.sqrt(area * ratio)).astype(np.int64)
    bh = np.rint(np.sqrt(area / ratio)).astype(np.int64)
    ok = (bw > 0) & (bw <= side[:, None]) & (bh > 0) & (bh <= side[:, None])
    by = _mulhi(tr[..., 2], np.maximum(side[:, None] - bh, 0).astype(np.uint64) + np.uint64(1))
    bx = _mulhi(tr[..., 3], np.maximum(side[:, None] - bw, 0).astype(np.uint64) + np.uint64(1))
    first = np.where(ok.any(axis=1), ok.argmax(axis=1), AUG_TRIES)
    rows, pick = np.arange(sid.size), np.minimum(first, AUG_TRIES - 1)
    hit = first < AUG_TRIES
    # the fallback of a side x side image: in_ratio = 1 lies inside [3/4, 4/3], so w = h = side, centred
    sel = lambda v, fb: np.where(hit, v[rows, pick], fb)
    return {"angle": angle, "flip": flip, "crop_side": side, "crop_top": top, "crop_left": left,
            "box_w": sel(bw, side), "box_h": sel(bh, side), "box_top": sel(by, 0), "box_left": sel(bx, 0), "tries": first,
            "area_frac": sel(frac, np.nan), "ratio": sel(ratio, np.nan)}


def _rotation_q16(angle, h_src, w_src):
    """int64 ``[B, 6]``: the Q16 coefficients with which PIL's ``rotate(angle, NEAREST)`` reads its source -- output pixel (X, Y) is source
    pixel ``((a0 X + a1 Y + a2) >> 16, (a3 X + a4 Y + a5) >> 16)``.  PIL forms the inverse matrix about the centre (w/2, h/2) in doubles,
    then ``FIX(v) = floor(65536 v + 1/2)`` of its entries, the offsets with the half-pixel terms folded in."""
    a = -np.radians(np.mod(np.asarray(angle, dtype=np.float64), 360.0))
    c, s = np.round(np.cos(a), 15), np.round(np.sin(a), 15)
    cx, cy = w_src / 2.0, h_src / 2.0
    m2 = (c * (-cx) + s * (-cy) + 0.0) + cx
    m5 = ((-s) * (-cx) + c * (-cy) + 0.0) + cy
    fix = lambda v: np.floor(v * 65536.0 + 0.5).astype(np.int64)
    return np.stack([fix(c), fix(s), fix(m2 + c * 0.5 + s * 0.5), fix(-s), fix(c), fix(m5 + (-s) * 0.5 + c * 0.5)], axis=1)


def augment_image_table(params: dict, src_index, src_hw) -> np.ndarray:
    """int32 ``[B, AUG_IMAGE_WORDS]``: the quantised row per sample that ``fc_augment_images`` reads, and the only thing
    ``augment_image_field`` reads of the draws: (source, a0 .. a5 of ``_rotation_q16``, crop left, crop top, crop side, box x0, box y0,
    box w, box h, flip, 0)."""
    src = np.asarray(src_index, dtype=np.int64).reshape(-1)
    hw = _src_hw(src_hw, src.size)
    rot = _rotation_q16(params["angle"], hw[:, 0], hw[:, 1])
    cols = [src, *rot.T, params["crop_left"], params["crop_top"], params["crop_side"], params["box_left"], params["box_top"],
            params["box_w"], params["box_h"], np.asarray(params["flip"]).astype(np.int64), np.zeros_like(src)]
    tab = np.stack([np.broadcast_to(np.asarray(c, dtype=np.int64), src.shape) for c in cols], axis=1)
    if tab.size and np.abs(tab).max() > 0x7fffffff:
        raise ValueError("augmentation table overflows 32 bits")
    return np.ascontiguousarray(tab.astype(np.int32))


def resize_taps(origin: int, extent: int, size: int, limit: int):
    """PIL's antialiased bilinear coefficients for resizing ``[origin, origin + extent)`` of an axis of ``limit`` pixels to ``size``,
    in integers: with ``D = 2 max(size, extent)`` and ``c = 2 size origin + (2 j + 1) extent`` (the centre of output j, times 2 size)
    the taps of output j are ``lo_j <= x < hi_j``, ``lo = max(0, floor((c - D + size) / (2 size)))``, ``hi = min(limit, floor((c + D +
    size) / (2 size)))``, with numerators ``n = max(0, D - |(2 x + 1) size - c|)`` -- a tent of half-width ``max(1, extent / size)``
    about the centre -- and the weight is ``n`` over the sum of the output's numerators.  Returns int64 ``(lo [size], hi [size],
    numerators [size, limit])`` (zero outside the taps)."""
    j = np.arange(size, dtype=np.int64)
    d = 2 * max(size, extent)
    c = 2 * size * origin + (2 * j + 1) * extent
    lo = np.maximum(0, (c - d + size) // (2 * size))
    hi = np.minimum(limit, (c + d + size) // (2 * size))
    x = np.arange(limit, dtype=np.int64)[None, :]
    n = np.maximum(0, d - np.abs((2 * x + 1) * size - c[:, None]))
    n = np.where((x >= lo[:, None]) & (x < hi[:, None]), n, 0)
    return lo, hi, n


def _source_bytes(src) -> np.ndarray:
    a = np.asarray(src)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (1, 3):
        raise ValueError(f"a source is a uint8 [H, W], [H, W, 1] or [H, W, 3] array, not {a.dtype} {a.shape}")
    return a


def augment_image_field(seed: int, sample_ids, sources, src_index, image_size, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), fill=-1.0,
                        params=None) -> np.ndarray:
    """fp64 ``[B, 3, S, S]``: the definition of what ``fc_augment_images`` writes for ``(seed, sample_ids[b])`` on
    ``sources[src_index[b]]`` (uint8 HWC arrays; one channel is replicated to three) -- upstream's ``image_transforms`` with the rotated
    image kept virtual:

    - ``R[Y, X]`` = the source at ``((a3 X + a4 Y + a5) >> 16, (a0 X + a1 Y + a2) >> 16)`` (row, column; ``augment_image_table``'s Q16
      coefficients, which are PIL's own for ``rotate(angle, NEAREST)``, 64-bit integer arithmetic), or ``fill`` outside the source;
    - the centre crop ``R[top : top + side, left : left + side]``;
    - PIL's antialiased bilinear resize of the box to ``S x S``: ``out = Wy R Wx^T`` with the rows of ``resize_taps`` -- a separable
      tent of half-width ``max(1, box / S)`` per axis, taps clamped to the centre crop (as ``Image.resize(..., box=)`` does; upstream
      crops first, so a tap that here reads the crop beyond the box's edge reads nothing there), weights normalised per output row
      and column;
    - the horizontal flip, then ``(v / 255 - mean) / std``.

    Only the weights are floating point, and they are continuous in the position, so no pixel of a comparison hangs on a rounding tie.
    ``fill`` (a scalar or three values) is in OUTPUT units: a tap outside the source contributes the byte value ``255 (fill std +
    mean)``; the default -1.0 is black under the default mean and std.  Upstream passes ``fill=means = [0.5, 0.5, 0.5]`` to a rotation
    of 8-bit PIL images, which is believed to truncate to byte 0, black; that belief cannot be checked without torchvision, which is why
    it is a parameter.  ``params``: the dict of ``augment_image_params`` with entries replaced (forced angles, flips, boxes)."""
    s = _check_aug_size(image_size)
    sid = np.asarray(sample_ids, dtype=np.int64).reshape(-1)
    src_index = np.asarray(src_index, dtype=np.int64).reshape(-1)
    if src_index.size != sid.size:
        raise ValueError(f"{src_index.size} source indices for {sid.size} sample ids")
    if src_index.size and (src_index.min() < 0 or src_index.max() >= len(sources)):
        raise ValueError(f"source index outside [0, {len(sources)})")
    srcs = [_source_bytes(a) for a in sources]
    hw = np.array([srcs[i].shape[:2] for i in src_index], dtype=np.int64).reshape(-1, 2)
    if params is None:
        params = augment_image_params(seed, sid, hw, s)
    tab = augment_image_table(params, src_index, hw).astype(np.int64)
    mean, std = np.broadcast_to(np.asarray(mean, np.float64), (3,)), np.broadcast_to(np.asarray(std, np.float64), (3,))
    fill_byte = 255.0 * (np.broadcast_to(np.asarray(fill, np.float64), (3,)) * std + mean)
    out = np.empty((sid.size, 3, s, s), dtype=np.float64)
    for b, row in enumerate(tab):
        a = srcs[row[0]]
        h_src, w_src = a.shape[:2]
        a0, a1, a2, a3, a4, a5, left, top, side, bx, by, bw, bh, flip = (int(v) for v in row[1:15])
        xs, ys = left + np.arange(side, dtype=np.int64)[None, :], top + np.arange(side, dtype=np.int64)[:, None]
        sx, sy = (a0 * xs + a1 * ys + a2) >> 16, (a3 * xs + a4 * ys + a5) >> 16
        inside = (sx >= 0) & (sx < w_src) & (sy >= 0) & (sy < h_src)
        px = a[np.clip(sy, 0, h_src - 1), np.clip(sx, 0, w_src - 1)].astype(np.float64)             # [side, side, C]
        px = np.broadcast_to(px, (side, side, 3))
        r = np.where(inside[:, :, None], px, fill_byte[None, None, :])
        _, _, nx = resize_taps(bx, bw, s, side)
        _, _, ny = resize_taps(by, bh, s, side)
        wx, wy = nx / nx.sum(axis=1, keepdims=True), ny / ny.sum(axis=1, keepdims=True)
        v = np.stack([wy @ r[:, :, c] @ wx.T for c in range(3)])
        if flip:
            v = v[:, :, ::-1]
        out[b] = (v / 255.0 - mean[:, None, None]) / std[:, None, None]
    return out


def augment_midi_params(seed: int, sample_ids, src_hw, image_size, random_roll=True) -> dict:
    """The draws of upstream's ``midi_transforms`` as ``[B]`` int64 arrays.  ``RandomRoll`` fires (``roll``) with p = 0.5 and then shifts
    by ``shift_x`` in [-(W // 2), W // 2] and ``shift_y`` in [-24, 24] (two octaves); despite its name it is
    ``PIL.Image.rotate(0, translate=(shift_x, shift_y))``, a translation with zero fill and nothing circular: the image moves right and
    down for positive shifts, ``out[y, x] = in[y - shift_y, x - shift_x]``.  ``RandomCrop(image_size)`` follows with ``crop_top`` uniform
    in [0, H - S] and ``crop_left`` in [0, W - S]."""
    s = _check_aug_size(image_size)
    sid = np.asarray(sample_ids, dtype=np.int64).reshape(-1)
    hw = _src_hw(src_hw, sid.size)
    h_src, w_src = hw[:, 0], hw[:, 1]
    if hw.size and hw.min() < s:
        raise ValueError(f"RandomCrop({s}) of a source smaller than that")
    head, crop = aug_words(seed, sid, 1, 0), aug_words(seed, sid, 1, 1)
    roll = ((head[:, 0] >> np.uint64(31)) == 0) & bool(random_roll)
    max_h = w_src // 2
    sx = _mulhi(head[:, 1], (2 * max_h + 1).astype(np.uint64)) - max_h
    sy = _mulhi(head[:, 2], 2 * AUG_MAX_V_SHIFT + 1) - AUG_MAX_V_SHIFT
    return {"roll": roll, "shift_x": np.where(roll, sx, 0), "shift_y": np.where(roll, sy, 0),
            "crop_top": _mulhi(crop[:, 0], (h_src - s + 1).astype(np.uint64)), "crop_left": _mulhi(crop[:, 1], (w_src - s + 1).astype(np.uint64))}


def augment_midi_table(params: dict, src_index) -> np.ndarray:
    """int32 ``[B, AUG_MIDI_WORDS]``: (source, shift x, shift y, crop left, crop top, 0, 0, 0), the row ``fc_augment_midi`` reads."""
    src = np.asarray(src_index, dtype=np.int64).reshape(-1)
    z = np.zeros_like(src)
    cols = [src, params["shift_x"], params["shift_y"], params["crop_left"], params["crop_top"], z, z, z]
    tab = np.stack([np.broadcast_to(np.asarray(c, dtype=np.int64), src.shape) for c in cols], axis=1)
    if tab.size and np.abs(tab).max() > 0x7fffffff:
        raise ValueError("augmentation table overflows 32 bits")
    return np.ascontiguousarray(tab.astype(np.int32))


def augment_midi_field(seed: int, sample_ids, sources, src_index, image_size, random_roll=True, grayscale=False, binary_thresh=0.3,
                       out_channels=None, params=None) -> np.ndarray:
    """fp32 ``[B, out_channels, S, S]``: what ``fc_augment_midi`` writes, bit for bit -- upstream's ``midi_transforms``: the translation
    and the crop of ``augment_midi_params`` (integers), ``ToTensor``'s ``byte / 255`` in fp32, optionally ``MyRGBToGrayscale`` -- the
    channel sum ``(u0 + u1) + u2`` in fp32, clamped to [0, 1] -- and, for ``binary_thresh > 0``, ``BinaryGate``: 1 where the fp32 value
    ``>=`` the threshold rounded to fp32, else 0, as torch compares.  ``out_channels`` (1 or 3; default 1 with ``grayscale``, else 3):
    the gray value goes to every output channel; otherwise output channel k is source channel k, channel 0 of a one-channel source."""
    s = _check_aug_size(image_size)
    sid = np.asarray(sample_ids, dtype=np.int64).reshape(-1)
    src_index = np.asarray(src_index, dtype=np.int64).reshape(-1)
    if src_index.size != sid.size:
        raise ValueError(f"{src_index.size} source indices for {sid.size} sample ids")
    if src_index.size and (src_index.min() < 0 or src_index.max() >= len(sources)):
        raise ValueError(f"source index outside [0, {len(sources)})")
    oc = int(out_channels) if out_channels is not None else (1 if grayscale else 3)
    if oc not in (1, 3):
        raise ValueError("out_channels is 1 or 3")
    srcs = [_source_bytes(a) for a in sources]
    hw = np.array([srcs[i].shape[:2] for i in src_index], dtype=np.int64).reshape(-1, 2)
    if params is None:
        params = augment_midi_params(seed, sid, hw, s, random_roll)
    tab = augment_midi_table(params, src_index).astype(np.int64)
    out = np.empty((sid.size, oc, s, s), dtype=np.float32)
    for b, row in enumerate(tab):
        a = srcs[row[0]]
        h_src, w_src, ch = a.shape
        ys = np.arange(s, dtype=np.int64)[:, None] + (row[4] - row[2])
        xs = np.arange(s, dtype=np.int64)[None, :] + (row[3] - row[1])
        inside = (ys >= 0) & (ys < h_src) & (xs >= 0) & (xs < w_src)
        px = np.where(inside[:, :, None], a[np.clip(ys, 0, h_src - 1), np.clip(xs, 0, w_src - 1)], 0)
        u = px.astype(np.float32) / np.float32(255.0)                                                # [S, S, C] fp32, one rounding
        if grayscale:
            g = u[:, :, 0] if ch == 1 else (u[:, :, 0] + u[:, :, 1]) + u[:, :, 2]
            v = np.broadcast_to(np.minimum(np.maximum(g, np.float32(0)), np.float32(1))[None], (oc, s, s))
        else:
            v = np.stack([u[:, :, k if ch == 3 else 0] for k in range(oc)])
        if binary_thresh > 0:
            v = (v >= np.float32(binary_thresh)).astype(np.float32)
        out[b] = v
    return out


# ---- codebook fitting (csrc/rvq_train.hip: fc_codebook_draws, fc_rvq_seed_codes, fc_rvq_kmeans, fc_rvq_train_step) ------------------------
# How the residual quantiser's codebooks learn without gradients (the EMA / k-means / dead-code configuration the reference builds its
# ResidualVQ with, flocoder/codecs.py:456-467; third-party algorithm, parity unpinned, stated here).  Per level l, with r the residuals
# entering the level ([N, D] fp32; r_0 = z, r_{l+1} = r_l - E_l[i_l] formed in fp32) and E [K, D] its codebook:
#   assign      i_n = argmin_k |r_n - E_k|^2, first index on ties; counts n_k, sums S_k = sum_{i_n = k} r_n, commitment sum_n |r_n - E_{i_n}|^2
#   k-means     means <- r_{pi(0 .. K-1)}; ``iters`` times: assign, mean_k <- S_k / n_k (an empty cluster keeps its mean); then
#               E = means, cluster_size = the last counts, embed_avg = E * cluster_size              (codebook_lloyd)
#   EMA step    cs <- cs + (1 - decay)(n - cs); A <- A + (1 - decay)(S - A); E_k <- A_k / ((cs_k + 1e-5) / (sum cs + K 1e-5) * sum cs),
#               evaluated in fp64 and rounded once to the buffers' fp32, sum cs in index order        (codebook_ema)
#   expiry      threshold > 0: the j-th code in index order with cs_k < threshold takes r_{pi(j)}; its cs_k = threshold and
#               A_k = E_k * threshold                                                                (codebook_expire)
#   loss        commitment_weight * commitment sum / (N D)
# pi is the permutation of [0, N) of (seed, level, draw_index)                                        (codebook_draws)
CODEBOOK_KEY_OFFSET = 0x43424F4F4B464954       # "CBOOKFIT"
CODEBOOK_MAX_N = 1 << 24
CODEBOOK_EPS = 1e-5


def codebook_draws(seed: int, level: int, draw_index: int, n: int, count=None) -> np.ndarray:
    """int64 ``[count]`` (default ``n``): slot j holds ``pi(j mod n)``, the bits of ``fc_codebook_draws``.  Two Philox4x32-10 blocks under
    key ``seed + CODEBOOK_KEY_OFFSET`` (mod 2^64) with counters ``(0, draw_index, level, n)`` and ``(1, draw_index, level, n)`` give the
    multipliers ``m_0..3`` and addends ``a_0..3`` of a bijection of the b-bit words (b >= 1 the smallest with 2^b >= n): four rounds of
    ``x <- (x (m_r | 1) + a_r) mod 2^b; x <- x xor (x >> ceil(b / 2))``.  A slot applies it until the value falls below n (cycle walking:
    expected under two applications), so slots 0 .. n-1 are a permutation of ``range(n)``: the draws are distinct, with no sort."""
    n = int(n)
    if not 1 <= n <= CODEBOOK_MAX_N:
        raise ValueError(f"n={n}: 1 .. 2^24 vectors")
    if not 0 <= int(draw_index) <= 0xffffffff:
        raise ValueError("draw_index is a 32-bit counter word")
    count = n if count is None else int(count)
    key = (int(seed) + CODEBOOK_KEY_OFFSET) & 0xffffffffffffffff
    ctr = np.array([[0, int(draw_index), int(level), n], [1, int(draw_index), int(level), n]], dtype=np.uint64)
    w = philox4x32(ctr, np.array([key & 0xffffffff, key >> 32], dtype=np.uint64)).astype(np.uint64)
    b = max(1, (n - 1).bit_length())
    mask, sh = np.uint64((1 << b) - 1), np.uint64((b + 1) // 2)
    x = np.arange(count, dtype=np.uint64) % np.uint64(n)
    todo = np.ones(count, dtype=bool)
    while todo.any():
        v = x[todo]
        for r in range(4):
            v = (v * (w[0, r] | np.uint64(1)) + w[1, r]) & mask
            v ^= v >> sh
        x[todo] = v
        todo[todo] = v >= np.uint64(n)
    return x.astype(np.int64)


def codebook_assign(r, means):
    """fp64: (index of the nearest mean, first on ties; squared distance to it; squared distance to the nearest other VALUE) per row."""
    r, means = np.asarray(r, dtype=np.float64), np.asarray(means, dtype=np.float64)
    d = np.zeros((len(r), len(means)))
    for c in range(r.shape[1]):                                       # one [N, K] plane at a time: no [N, K, D] temporary
        d += (r[:, c, None] - means[None, :, c]) ** 2
    i = d.argmin(axis=1)
    best = d[np.arange(len(r)), i]
    nxt = np.where(d <= best[:, None], np.inf, d).min(axis=1)
    return i, best, nxt


def codebook_sums(r, idx, k: int):
    """(counts int64 [K], sums fp64 [K, D]) of the rows of r by their index."""
    r = np.asarray(r, dtype=np.float64)
    counts = np.bincount(idx, minlength=k).astype(np.int64)
    sums = np.zeros((k, r.shape[1]), dtype=np.float64)
    np.add.at(sums, idx, r)
    return counts, sums


def codebook_lloyd(data, init, iters: int):
    """``iters`` Lloyd iterations in fp64 from the means ``init``: (means, the last iteration's counts, the objective of every iteration =
    the sum of squared distances to the means the rows were assigned to, before the update).  An empty cluster keeps its mean."""
    data, means = np.asarray(data, dtype=np.float64), np.array(init, dtype=np.float64)
    counts, obj = np.zeros(len(means), dtype=np.int64), []
    for _ in range(int(iters)):
        i, best, _ = codebook_assign(data, means)
        counts, sums = codebook_sums(data, i, len(means))
        obj.append(best.sum())
        full = counts > 0
        means[full] = sums[full] / counts[full, None]
    return means, counts, np.array(obj)


def codebook_ema(cs, avg, counts, sums, decay: float, dtype=np.float32):
    """The EMA step of one level: (cluster_size, embed_avg, embed).  Evaluated in fp64; ``dtype`` = fp32 rounds where the device stores
    (cluster_size and embed_avg once each, and the codebook from the ROUNDED buffers), fp64 is the published lines as they stand."""
    om = 1.0 - float(decay)
    cs, avg = np.asarray(cs, dtype=np.float64), np.asarray(avg, dtype=np.float64)
    cs = (cs + om * (np.asarray(counts, dtype=np.float64) - cs)).astype(dtype)
    avg = (avg + om * (np.asarray(sums, dtype=np.float64) - avg)).astype(dtype)
    c64 = cs.astype(np.float64)
    tot = float(np.cumsum(c64)[-1])                                   # in index order
    smoothed = (c64 + CODEBOOK_EPS) / (tot + len(c64) * CODEBOOK_EPS) * tot
    return cs, avg, (avg.astype(np.float64) / smoothed[:, None]).astype(dtype)


def codebook_expire(cs, avg, embed, residuals, threshold: float, seed: int, level: int, draw_index: int):
    """Dead-code expiry on fp32 buffers (copies returned, with the indices of the replaced codes): code k with ``cs_k < threshold`` is
    dead; the j-th dead code in index order takes row ``pi(j)`` of ``residuals`` (this level's fp32 input)."""
    cs, avg, embed = (np.array(a, dtype=np.float32) for a in (cs, avg, embed))
    thr = np.float32(threshold)
    dead = np.flatnonzero(cs < thr) if thr > 0 else np.zeros(0, dtype=np.int64)
    if dead.size:
        pick = codebook_draws(seed, level, draw_index, len(residuals), dead.size)
        embed[dead] = np.asarray(residuals, dtype=np.float32)[pick]
        cs[dead] = thr
        avg[dead] = embed[dead] * thr
    return cs, avg, embed, dead
