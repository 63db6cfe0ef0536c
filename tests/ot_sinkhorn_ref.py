"""NumPy / SciPy fp64 restatement of the entropic OT plan solver (csrc/ot_plan.hip, ot_sinkhorn_kernel), of the plan sampler
(ot_sample_kernel) and of the plan-to-permutation sweep (ot_sweep_kernel<true>), the certificate the GPU tests hold the device's plan
to, and the cases both test files use (same generators, same seeds).

The solver: POT's sinkhorn_knopp in the log domain, uniform marginals.  f = g = reg log(1/B); per iteration
g_j = reg (log(1/B) - LSE_i((f_i - C_ij)/reg)) then f_i = reg (log(1/B) - LSE_j((g_j - C_ij)/reg)); after every 10th iteration
err = |colsum(P) - 1/B|_2 with P_ij = exp((f_i + g_j - C_ij)/reg); stop when err < stop_thr or at max_iter (rounded up to a multiple of 10).

The certificate.  A matrix of Gibbs form P_ij = exp((f_i + g_j - C_ij)/reg) is the entropic optimum for ITS OWN marginals (the first-order
conditions of the strictly convex problem are exactly that form), so a plan is checked by (a) its form, entry by entry against the
returned duals and cost, (b) its column marginal's distance from 1/B, (c) its row marginal's; neither POT nor torchcfm is needed.
(b) and (c) are evaluated on the Gibbs form in fp64: the stored plan is fp32, whose rounding (2^-24 per entry) is what (a) bounds.

The sampler: pair k inverts the plan's cdf (cells in row-major order) at u_k (flocoder_amd.noise.plan_uniforms), as
np.random.choice(p.size, p=p/p.sum()) does: searchsorted(cdf, u cdf[-1], side="right"), clamped to the last cell.  The device searches
two levels -- rows by the running sum of the row sums, then inside the row -- with every sum sequential in fp64; `sample_two_level`
restates that bit for bit, `sample_flat` is the one-level textbook form it is compared with."""
import functools

import numpy as np
from scipy.special import logsumexp

import ot_exact_ref as X

FLT_MIN = float(np.finfo(np.float32).tiny)
LDS_B = 192                                           # SKP_LDS_B in csrc/ot_plan.hip: the matrix lives in LDS up to this batch


# ---- the solver -----------------------------------------------------------------------------------------------------------------
def round_iters(max_iter):
    return (int(max_iter) + 9) // 10 * 10


def col_err(c, f, g, reg):
    """|colsum(P) - 1/B|_2 of the Gibbs form."""
    p = np.exp((f[:, None] + g[None, :] - c) / reg)
    return float(np.sqrt(((p.sum(0) - 1.0 / c.shape[0]) ** 2).sum()))


def sinkhorn(cost, reg, max_iter=1000, stop_thr=1e-9, trace=None):
    """(plan fp64 [B,B], f, g, iterations, converged, err).  ``trace``: a list that receives (iteration, err) of every check."""
    c = X.clean(cost).astype(np.float64)
    n = c.shape[0]
    lb = -np.log(float(n))
    f = np.full(n, reg * lb)
    g = np.full(n, reg * lb)
    it, err, conv = 0, np.inf, False
    for it in range(1, round_iters(max_iter) + 1):
        g = reg * (lb - logsumexp((f[:, None] - c) / reg, axis=0))
        f = reg * (lb - logsumexp((g[None, :] - c) / reg, axis=1))
        if it % 10 == 0:
            err = col_err(c, f, g, reg)
            if trace is not None:
                trace.append((it, err))
            if err < stop_thr:
                conv = True
                break
    return np.exp((f[:, None] + g[None, :] - c) / reg), f, g, it, conv, err


def sinkhorn_knopp(cost, reg, iterations):
    """Kernel-form Sinkhorn-Knopp as POT writes it, for a fixed number of iterations: (f, g) = reg log of the scalings."""
    c = np.asarray(cost, dtype=np.float64)
    n = c.shape[0]
    k = np.exp(-c / reg)
    u = np.full(n, 1.0 / n)
    v = np.full(n, 1.0 / n)
    for _ in range(iterations):
        v = (1.0 / n) / (k.T @ u)
        u = (1.0 / n) / (k @ v)
    return reg * np.log(u), reg * np.log(v)


def certificate(plan32, cost, f, g, reg):
    """On the device's outputs, in fp64: {"form": the largest |P - E| / E over entries with E >= FLT_MIN, E the Gibbs form (0 if none),
    "col": |colsum(E) - 1/B|_2, "row": max |rowsum(E) - 1/B|, "cost": <P, C>}."""
    c = np.asarray(cost, dtype=np.float64)
    e = np.exp((np.asarray(f)[:, None] + np.asarray(g)[None, :] - c) / reg)
    p = np.asarray(plan32, dtype=np.float64)
    big = e >= FLT_MIN
    form = float((np.abs(p - e)[big] / e[big]).max()) if big.any() else 0.0
    n = c.shape[0]
    return {"form": form, "col": float(np.sqrt(((e.sum(0) - 1.0 / n) ** 2).sum())), "row": float(np.abs(e.sum(1) - 1.0 / n).max()),
            "cost": float((p * c).sum()), "small_ok": bool((p[~big] < FLT_MIN).all())}


def cost_bounds(cost):
    """(lower, upper) of <P, C> over plans with uniform marginals that the entropic optimum must respect: the assignment optimum / B
    (Birkhoff: the plans are the convex hull of the permutation matrices / B) and mean(C) (the uniform plan has maximal entropy, so the
    entropic optimum cannot cost more)."""
    from scipy.optimize import linear_sum_assignment
    c = np.asarray(cost, dtype=np.float64)
    r, k = linear_sum_assignment(c)
    return float(c[r, k].sum()) / c.shape[0], float(c.mean())


# ---- the sampler ----------------------------------------------------------------------------------------------------------------
def sample_flat(plan, u):
    """(i, j) by one searchsorted over the flat fp64 cdf."""
    p = np.asarray(plan, dtype=np.float64)
    cdf = np.cumsum(p.ravel())
    idx = np.minimum(np.searchsorted(cdf, u * cdf[-1], side="right"), p.size - 1)
    return np.divmod(idx.astype(np.int64), p.shape[1])


def sample_two_level(plan, u):
    """(i, j, ok) as the device forms them.  ok False: the plan's sum is not positive and finite, the pairs are (k mod B, k mod B)."""
    p = np.asarray(plan, dtype=np.float32).astype(np.float64)
    n = p.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        within = np.cumsum(p, axis=1)                     # sequential, ascending j
        rows = np.cumsum(within[:, -1])                   # sequential, ascending i
    total = rows[-1]
    k = np.arange(len(u), dtype=np.int64)
    if not (total > 0.0 and np.isfinite(total)):
        return k % n, k % n, False
    t = u * total
    i = np.minimum(np.searchsorted(rows, t, side="right"), n - 1)
    tp = t - np.where(i > 0, rows[np.maximum(i - 1, 0)], 0.0)
    j = np.minimum((within[i] <= tp[:, None]).sum(1), n - 1)
    # the device takes the FIRST j whose running sum exceeds t'; with non-negative entries the running sum is monotone and that is the count above
    return i.astype(np.int64), j.astype(np.int64), True


def plan_pairing(plan):
    """Upstream's vanilla conversion: for rows in order the largest entry among the unused columns, ties to the lowest column."""
    p = np.asarray(plan, dtype=np.float32)
    used = np.zeros(p.shape[1], dtype=bool)
    perm = np.empty(p.shape[0], dtype=np.int64)
    for i in range(p.shape[0]):
        row = np.where(used, -np.inf, p[i])
        j = int(np.argmax(row))                           # first maximum
        perm[i] = j
        used[j] = True
    return perm


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# (B, D, reg, normalise, max_iter): the wave tail (1, 2, 7, 65), both homes of the matrix (192 | 193), more rows than waves, the size limit
CASES = [(1, 8, 0.05, True, 1000), (2, 8, 0.05, True, 1000), (7, 16, 0.05, True, 1000), (64, 32, 0.05, True, 1000),
         (65, 32, 0.05, True, 1000), (LDS_B, 16, 0.05, True, 1000), (LDS_B + 1, 16, 0.05, True, 1000), (256, 64, 0.05, True, 1000),
         (128, 32, 0.01, True, 1000), (1024, 8, 0.05, True, 20)]
STUCK_CASES = [(64, 32, 0.002, True, 1000), (64, 4, 0.1, False, 1000)]          # no convergence within max_iter
SAMPLE_CASES = [(8, 16, 0.05), (64, 32, 0.05), (193, 16, 0.05), (64, 32, 0.002)]  # the last: a near-permutation plan
STOP_THR = 1e-9


def points(B, D):
    return X.pair_case(B, D)


def normalise(c):
    """fp32 matrix / its largest non-sentinel entry (left alone when that is not positive), as ot_normalize_kernel."""
    c = X.clean(c)
    fin = c < np.float32(X.FLT_MAX)
    m = c[fin].max() if fin.any() else np.float32(0)
    if not m > 0:
        return c
    out = c.copy()
    out[fin] = c[fin] / m
    return out


@functools.lru_cache(maxsize=None)
def host_cost(B, D, normalised):
    """The CPU stand-in for the matrix the device's solver sees (fp32 squared distances, optionally divided by their maximum)."""
    c = X.sqdist32(*points(B, D))
    return normalise(c) if normalised else c


@functools.lru_cache(maxsize=None)
def host_solution(case):
    """(plan, f, g, iterations, converged, err, trace) of the restatement on ``host_cost``; computed once per session."""
    B, D, reg, normalised, max_iter = case
    trace = []
    out = sinkhorn(host_cost(B, D, normalised), reg, max_iter, STOP_THR, trace)
    return out + (tuple(trace),)


def equal_matrix(B, value=3.0):
    return X.equal_matrix(B, value)
