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
