"""fp64 references, derived error bounds and shared seeded inputs for the kernels that close a training step (test infrastructure; the
product never imports it): the prologue (``fc_flow_prepare[_rows]``, ``fc_flow_interp``), the loss (``fc_mse_loss_grad[_scaled]``),
the clip (``fc_grad_clip_coef``) and Adam + EMA (``fc_adam_ema_step[_guarded]``).

References are plain float64 restatements on the fp32 inputs promoted to double.  Hyper-parameters are read as torch reads them:
Python doubles, ``1 - beta`` formed in double -- NOT the float a C ABI may happen to carry.  Adam and the clip are not restated here:
``oracle.train_oracle`` (held to ``torch.optim.Adam`` / ``clip_grad_norm_`` by tests/test_step_pieces_cpu.py) runs on float64.

Bounds.  ``U = 2^-24`` is fp32's unit roundoff; k rounded operations in a row cost ``gamma(k) = k U / (1 - k U)`` (the rigorous form
of "k U").  Each bound below counts the rounded operations of the straightforward fp32 evaluation -- the kernels' and torch's own --
and none is fitted to what a kernel returns; tests/test_step_pieces_cpu.py asserts that torch's fp32 evaluation (and, for the two
reductions, an fp32 emulation of the kernels' partition) stays inside every one of them on every input set the GPU test uses.

  v* = g - s     bit-equal to fp32 ``g - s`` (one correctly rounded operation)
  t, time        bit-equal to ``flocoder_amd.sampling.warp_time`` on the CPU at s = 0.5, and to ``t * t_scale``; ``t_bound`` at other s
  x              gamma(4) (|(1-t) s| + |t g|): 1 - t, two products, one sum (FMA contraction may differ from torch: no bit-equality)
  dv             gamma(4) |ref|: v - v*, the rounded 2 scale / n, one product
  loss, norm^2   relative gamma(K + D): a sum of non-negative terms, K sequential adds per thread, D the remaining depth
  norm, coef     gamma((K + D) / 2 + 3) relative where the clip is active (sqrt halves the sum's error; sqrt, norm + 1e-6, the
                 division: 3 more); exactly 1.0f where it is not
  m'             gamma(4) (|m| + |coef g|)
  v'             gamma(4) v'_ref
  p'             2 U |p'_ref| + (lr / bc1) bound(m') / denom_ref + 8 U |update_ref|
  ema'           gamma(4) (|ema| + |p'_ref|) + bound(p')

The depth D, counted from ``block_sum`` (csrc/stats_dev.h) and the kernels of csrc/backward.hip: a thread's K = ceil(n / 65536) adds
(256 blocks x 256 threads, grid-stride); ``block_sum`` is 6 butterfly adds (offsets 32, 16, 8, 4, 2, 1 inside a 64-lane wave) and 3
adds over the 4 waves' totals = 9, run twice (every block, then the 256 block totals) = 18.  MSE: the term ``(v - v*)^2`` is one
subtraction (its relative error counts twice in the square) and one product = 3, the final scale is the rounded ``scale / n`` and
one product = 2: D_MSE = 3 + 18 + 2 = 23.  Sum of squares: one product per term, nothing after the trees: D_SUMSQ = 1 + 18 = 19.
``fc_mse_loss_grad_scaled`` adds its share to a running scalar: one more U of the accumulated value per call.
"""
import math

import torch

from oracle import train_oracle as to

U = 2.0 ** -24
RED_THREADS = 256 * 256           # kRedBlocks x 256 threads, grid-stride
TREE = 2 * (6 + 3)                # two block_sum trees
D_MSE = 3 + TREE + 2
D_SUMSQ = 1 + TREE
F32, F64 = torch.float32, torch.float64


def gamma(k):
    return k * U / (1.0 - k * U)


def red_k(n):
    """Sequential adds of one thread over a range of n elements."""
    return -(-int(n) // RED_THREADS)


# ---- prologue -----------------------------------------------------------------------------------------------------------------------
def warp_coeffs(s):
    return 4 * (1 - s), 6 * (s - 1), 3 - 2 * s


def gather_rows(batch, pairing, first_row, target_rows):
    """(rows [batch] int64 of the target each output row reads, pairing_flag): an entry outside [0, target_rows) falls back to the
    row's own target first_row + b and sets bit 1."""
    own = first_row + torch.arange(batch, dtype=torch.int64)
    if pairing is None:
        return own, 0
    bad = (pairing < 0) | (pairing >= target_rows)
    return torch.where(bad, own, pairing), (2 if bool(bad.any()) else 0)


def prepare(src, tgt, u, t_eps, warp_s, t_scale, pairing=None, ids=None, n_classes=0, first_row=0, target_rows=None, t_for_x=None):
    """fp64 prologue of train_flow.py:346-357.  src [batch, per], tgt [target_rows, per], u [batch] (fp32 or fp64; promoted).
    ``t_for_x``: the fp32 t the interpolation stage was handed (the device's own t output, gated on its own): x is then that
    stage's fp64 restatement, so its bound needs no term for t's error.  Returns a dict of float64 tensors and the flag bits."""
    batch = src.shape[0]
    target_rows = tgt.shape[0] if target_rows is None else target_rows
    a3, a2, a1 = warp_coeffs(warp_s)
    t0 = u.to(F64) * (1 - t_eps) + t_eps
    t = a3 * t0 ** 3 + a2 * t0 ** 2 + a1 * t0
    rows, flag = gather_rows(batch, pairing, first_row, target_rows)
    if ids is not None and bool(((ids < 0) | (ids >= n_classes)).any()):
        flag |= 1
    s, g = src.to(F64), tgt.to(F64)[rows]
    tx = (t if t_for_x is None else t_for_x.to(F64)).reshape(-1, 1)
    return {"t": t, "time": t * t_scale, "x": (1 - tx) * s + tx * g, "v": g - s, "flag": flag, "rows": rows,
            "x_bound": gamma(4) * (((1 - tx) * s).abs() + (tx * g).abs())}


def t_bound(u, t_eps, warp_s):
    """|t_fp32 - t_fp64| for t = warp(u (1 - eps) + eps): t0 carries the rounded 1 - eps and eps, one product and one sum, at most
    gamma(4) (|u| + eps), which the polynomial passes on through |w'(t0)|; the three terms carry their rounded coefficient, the
    powers (t0^2: 1, t0^3: 2) and one product, and the two sums one rounding of the partial sums each: at most gamma(6) of the
    terms' magnitudes together."""
    a3, a2, a1 = warp_coeffs(warp_s)
    t0 = u.to(F64) * (1 - t_eps) + t_eps
    slope = (3 * a3 * t0 ** 2 + 2 * a2 * t0 + a1).abs()
    return slope * gamma(4) * (u.to(F64).abs() + t_eps) + gamma(6) * (abs(a3) * t0 ** 3 + abs(a2) * t0 ** 2 + abs(a1) * t0)


def interp(src, tgt, t):
    """fc_flow_interp in fp64: (x, v*, bound(x))."""
    s, g, tt = src.to(F64), tgt.to(F64), t.to(F64).reshape(-1, 1)
    return (1 - tt) * s + tt * g, g - s, gamma(4) * (((1 - tt) * s).abs() + (tt * g).abs())


# ---- loss ---------------------------------------------------------------------------------------------------------------------------
def mse(v, tgt, scale=1.0):
    """(loss, dv) in fp64: scale * mean((v - v*)^2) and scale * 2 (v - v*) / n.  ``scale`` as the caller holds it (a double)."""
    d = v.to(F64).reshape(-1) - tgt.to(F64).reshape(-1)
    return scale * (d * d).mean(), scale * 2.0 * d / d.numel()


def loss_rel_bound(n, extra=0):
    return gamma(red_k(n) + D_MSE + extra)


def dv_bound(dv_ref):
    return gamma(4) * dv_ref.abs()


# ---- clip ---------------------------------------------------------------------------------------------------------------------------
def clip(g, g2, max_norm):
    """(norm, coef) in fp64 over one or two ranges: the oracle's grad_norm / clip_coef."""
    grads = {"a": g.to(F64)}
    if g2 is not None:
        grads["b"] = g2.to(F64)
    norm = to.grad_norm(grads)
    return norm, to.clip_coef(norm, max_norm)


def norm_rel_bound(n, n2=0):
    """Relative bound of the norm, and of the coefficient where the clip is active."""
    return gamma((red_k(n) + red_k(n2) + D_SUMSQ) / 2 + 3)


coef_rel_bound = norm_rel_bound


# ---- Adam + EMA ---------------------------------------------------------------------------------------------------------------------
def clipped(g, coef):
    """The gradient Adam reads: clip_grad_norm_ multiplies p.grad by the coefficient in place, so torch's Adam is handed the fp32
    product g * coef, one correctly rounded operation (as v* = g - s in the prologue).  It is an fp32 input of the Adam arithmetic
    and is promoted as such; a reference on the unrounded product would charge Adam's bounds for a rounding that is not Adam's
    (at step 1 with zero moments exp_avg_sq = (1 - beta2) gv^2 would carry 5 roundings, and torch's own fp32 Adam misses
    gamma(4) on such inputs)."""
    return g.to(F32) * torch.tensor(coef, dtype=F32)


def adam_ema(p, g, m, v, ema, coef, lr, b1, b2, eps, step, decay, apply_adam=True, dtype=F64):
    """One torch.optim.Adam step on clipped(g, coef) with bias corrections for ``step`` (1-based), then the EMA: the oracle on ``dtype``
    tensors (float64: the reference; float32: torch's own fp32 arithmetic).  Returns (p', m', v', ema') as float64."""
    sd = {"w": p.to(dtype).clone()}
    st = {"m": {"w": m.to(dtype).clone()}, "v": {"w": v.to(dtype).clone()}, "step": {"w": step - 1},
          "ema": {"w": ema.to(dtype).clone()}, "ema_decay": decay}
    # without a gradient the oracle still wants a norm to clip by: "-" is no parameter of sd and feeds the norm alone
    grads = {"w": clipped(g, coef).to(dtype)} if apply_adam else {"w": None, "-": torch.zeros(1, dtype=dtype)}
    to.adam_ema_step(sd, grads, st, lr=lr, betas=(b1, b2), eps=eps, max_norm=float("inf"))
    return sd["w"].to(F64), st["m"]["w"].to(F64), st["v"]["w"].to(F64), st["ema"]["w"].to(F64)


def adam_bounds(g, m, ema, coef, lr, b1, b2, eps, step, ref, apply_adam=True):
    """Elementwise bounds (bp, bm, bv, be) around ``ref`` = adam_ema(...) in fp64."""
    p_ref, m_ref, v_ref, _ = ref
    e = ema.to(F64)
    if not apply_adam:
        z = torch.zeros_like(p_ref)
        return z, z, z, gamma(4) * (e.abs() + p_ref.abs())
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    den = v_ref.sqrt() / math.sqrt(bc2) + eps
    bm = gamma(4) * (m.to(F64).abs() + clipped(g, coef).to(F64).abs())
    bv = gamma(4) * v_ref
    upd = lr / bc1 * m_ref.abs() / den
    bp = 2 * U * p_ref.abs() + lr / bc1 * bm / den + 8 * U * upd
    return bp, bm, bv, gamma(4) * (e.abs() + p_ref.abs()) + bp


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; a zero bound demands equality (ratio 0 when met, inf when not)."""
    err = (got.to(F64) - ref.to(F64)).abs().reshape(-1)
    bound = bound.to(F64).reshape(-1) if torch.is_tensor(bound) else torch.full_like(err, float(bound))
    if err.numel() == 0:
        return 0.0
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


# ---- fp32 emulation of the kernels' reduction partition -----------------------------------------------------------------------------
def _block_sum32(x):
    """block_sum of csrc/stats_dev.h over the last axis (256 lanes) in fp32: xor butterflies inside each 64-lane wave, then the four
    wave totals added left to right."""
    lane = torch.arange(256)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[..., lane ^ o]
    return ((x[..., 0] + x[..., 64]) + x[..., 128]) + x[..., 192]


def partition_sum32(*term_ranges):
    """The fp32 sum the two-stage reductions form: every range's terms (fp32, already squared) go to 65536 threads grid-stride, each
    thread adds its terms in order (range after range), then block_sum per block and block_sum over the 256 block totals."""
    acc = torch.zeros(RED_THREADS, dtype=F32)
    for terms in term_ranges:
        terms = terms.reshape(-1)
        k = red_k(terms.numel())
        padded = torch.zeros(k * RED_THREADS, dtype=F32)
        padded[:terms.numel()] = terms
        for row in padded.reshape(k, RED_THREADS):
            acc = acc + row
    return _block_sum32(_block_sum32(acc.reshape(256, 256)))


# ---- shared, seeded inputs (no denormals) -------------------------------------------------------------------------------------------
T_EPS, T_SCALE, N_CLASSES = 1e-3, 999.0, 10
PER = (1, 3, 1023, 1024, 1025, 70001)
BATCH = (1, 5, 16)
WARP_S = (0.5, 0.0, 1.0, 1.5)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, gen):
    x = torch.randn(shape, generator=gen)
    return torch.where(x.abs() < 1e-30, torch.full_like(x, 1e-30), x)


def prologue_cases():
    """Every (per, batch) once, the variants rotating so that each warp_s, pairing kind, class-id kind and both forms occur with
    several shapes: dicts with src [batch, per], tgt [target_rows, per], u [batch] (exactly 0 and 1 included), pairing / ids (int64
    or None), use_flag, first_row, target_rows, rows_form."""
    out = []
    i = 0
    for per in PER:
        for batch in BATCH:
            gen = _gen(1000 + i)
            rows_form = i % 2 == 1
            first_row, target_rows = (2, batch + 5) if rows_form else (0, batch)
            u = torch.rand(batch, generator=gen)
            u[0] = float(i % 2)
            if batch > 1:
                u[-1], u[1] = 1.0, 0.0
            pk = ("none", "perm", "repeats", "bad")[(i // 2 + i) % 4]
            if pk == "none":
                pairing = None
            elif pk == "perm":
                pairing = torch.randperm(target_rows, generator=gen)[:batch].clone()
            elif pk == "repeats":
                pairing = torch.randint(0, target_rows, (batch,), generator=gen)
                pairing[-1] = pairing[0]
            else:
                pairing = torch.randint(0, target_rows, (batch,), generator=gen)
                pairing[0] = -1 if i % 4 < 2 else target_rows
                if batch > 1:
                    pairing[-1], pairing[0] = target_rows, -1
            ik = ("ok", "high", "neg", "none", "bad_noflag")[i % 5]
            ids = None if ik == "none" else torch.randint(0, N_CLASSES, (batch,), generator=gen)
            if ik in ("high", "bad_noflag"):
                ids[batch // 2] = N_CLASSES
            if ik == "neg":
                ids[batch // 2] = -1
            out.append({"name": f"per{per}-b{batch}-s{WARP_S[i % 4]}-{pk}-{ik}-{'rows' if rows_form else 'plain'}", "per": per,
                        "batch": batch, "warp_s": WARP_S[i % 4], "src": _randn((batch, per), gen), "tgt": _randn((target_rows, per), gen),
                        "u": u, "pairing": pairing, "ids": ids, "use_flag": ik != "bad_noflag", "first_row": first_row,
                        "target_rows": target_rows, "rows_form": rows_form})
            i += 1
    return out


LOSS_N = (1, 255, 65536, 65537, 2 ** 20 + 3)


def loss_cases():
    """(name, v, tgt) for every n, plain and with a large common offset (v, tgt ~ 100 + 1e-3 noise)."""
    out = []
    for j, n in enumerate(LOSS_N):
        gen = _gen(2000 + j)
        out.append((f"n{n}-plain", _randn(n, gen), _randn(n, gen)))
        out.append((f"n{n}-offset", 100 + 1e-3 * _randn(n, gen), 100 + 1e-3 * _randn(n, gen)))
    return out


MICRO_ROWS, MICRO_PER = (3, 1, 2), 4099


def micro_case():
    gen = _gen(2100)
    rows = sum(MICRO_ROWS)
    return _randn((rows, MICRO_PER), gen), _randn((rows, MICRO_PER), gen)


CLIP_N = (1, 4099, 2 ** 20 + 3)
CLIP_MAX_NORM = 2.0


def clip_cases():
    """(name, g, g2 or None, max_norm): norms at 0.5 and 3 max_norm for every n with and without a second range of odd length, and an
    all-zero gradient."""
    out = []
    for j, n in enumerate(CLIP_N):
        for k, factor in enumerate((0.5, 3.0)):
            for n2 in (0, 777):
                gen = _gen(3000 + 10 * j + 2 * k + (n2 > 0))
                g, g2 = _randn(n, gen), (_randn(n2, gen) if n2 else None)
                norm = clip(g, g2, CLIP_MAX_NORM)[0]
                s = factor * CLIP_MAX_NORM / float(norm)
                out.append((f"n{n}-x{factor}-second{n2}", (g.to(F64) * s).to(F32), None if g2 is None else (g2.to(F64) * s).to(F32), CLIP_MAX_NORM))
    out.append(("zeros", torch.zeros(4099), None, CLIP_MAX_NORM))
    return out


B1, B2, EPS, DECAY = 0.9, 0.999, 1e-8, 0.999
ADAM_N = (1, 255, 257, 4099, 2048 * 256 + 4099)
ADAM_STATES = (("zero", 1), ("nonzero", 1), ("nonzero", 7), ("nonzero", 100000))
ADAM_LR = (1e-4, 1e-3)
ADAM_COEF = (1.0, 0.37)
ADAM_GSCALE = (1.0, 1e-4, 1e-9)


def adam_inputs(n, state, gscale, seed):
    """p, g, m, v, ema (fp32): gradients over three decades below ``gscale`` with |g| >= 1e-13 (g^2 (1 - beta2) stays above 1e-30),
    moments of matching size (or zero), an EMA close to p."""
    gen = _gen(seed)
    p = _randn(n, gen) * 0.1
    g = _randn(n, gen) * gscale * torch.logspace(-3, 0, n)
    g = torch.where(g.abs() < 1e-13, torch.full_like(g, 1e-13), g)
    m = _randn(n, gen) * gscale * 0.3
    v = ((_randn(n, gen) * gscale).square() * torch.rand(n, generator=gen)).clamp_min(1e-30)
    if state == "zero":
        m, v = torch.zeros(n), torch.zeros(n)
    return p, g, m, v, p + _randn(n, gen) * 1e-3


def adam_cases():
    """dicts(name, n, state, step, lr, coef, gscale, seed): all sixteen (state/step, lr, coef) combinations at every n below the
    grid's cap, four of them (every value of each occurring) above it."""
    out = []
    c = 0
    for n in ADAM_N:
        for si, (state, step) in enumerate(ADAM_STATES):
            for li, lr in enumerate(ADAM_LR):
                for ci, coef in enumerate(ADAM_COEF):
                    if n == ADAM_N[-1] and (li, ci) != (si % 2, (si // 2) % 2):
                        continue
                    out.append({"name": f"n{n}-{state}-step{step}-lr{lr}-coef{coef}", "n": n, "state": state, "step": step, "lr": lr,
                                "coef": coef, "gscale": ADAM_GSCALE[c % 3], "seed": 4000 + c})
                    c += 1
    return out


HORIZON_STEPS, HORIZON_N, HORIZON_MAX_NORM, HORIZON_LR = 200, 4099, 3.0, 1e-3


def horizon_inputs():
    """p0 [n] and the gradient sequence [steps, n]: magnitudes 1e-7 .. 1 across the vector, an amplitude that moves the norm to both
    sides of HORIZON_MAX_NORM."""
    gen = _gen(5000)
    p0 = _randn(HORIZON_N, gen) * 0.1
    scale = torch.logspace(-7, 0, HORIZON_N)
    amp = torch.tensor([0.3 + 0.2 * math.sin(s) for s in range(1, HORIZON_STEPS + 1)]).reshape(-1, 1)
    g = _randn((HORIZON_STEPS, HORIZON_N), gen) * scale * amp + 0.05 * scale
    return p0, torch.where(g.abs() < 1e-13, torch.full_like(g, 1e-13), g)


def horizon_oracle(p0, grads, dtype):
    """The oracle's clip -> Adam -> EMA loop on ``dtype``; returns (p, m, v, ema) as float64 and the per-step norms."""
    sd = {"w": p0.to(dtype).clone()}
    st = to.new_state(sd, DECAY)
    norms = [float(to.adam_ema_step(sd, {"w": g.to(dtype)}, st, lr=HORIZON_LR, betas=(B1, B2), eps=EPS, max_norm=HORIZON_MAX_NORM)) for g in grads]
    return (sd["w"].to(F64), st["m"]["w"].to(F64), st["v"]["w"].to(F64), st["ema"]["w"].to(F64)), norms


def horizon_figures(got, ref):
    """(worst relative deviation of exp_avg_sq, worst absolute deviation of exp_avg, of p, of ema) from the fp64 loop."""
    return (float(((got[2] - ref[2]).abs() / ref[2]).max()), float((got[1] - ref[1]).abs().max()),
            float((got[0] - ref[0]).abs().max()), float((got[3] - ref[3]).abs().max()))
