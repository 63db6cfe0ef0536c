"""fp64 restatement of codebook fitting (flocoder_amd/noise.py, "codebook fitting") for the tests: the level walk in the device's fp32
order, the training step and the Lloyd iteration fed with given indices, and the accumulation bound of csrc/rvq_train.hip.

ACCUMULATION BOUND (derived at the head of csrc/rvq_train.hip).  The device adds each residual component as the 64-bit integer
rint(r 2^s), s = 38 - e, where 2^e is the power of two above M = max|z| + sum_{l < last} max|E_l|; one conversion errs by at most
2^-(s+1) = 2^(e-39), so a sum over n_k vectors errs by at most n_k 2^(e-39) and a mean by 2^(e-39) -- integer addition is exact and
order-free, nothing else enters.  On top of that a stored fp32 value may round the other way: one ulp of the restatement's value.
"""
import numpy as np

from flocoder_amd import noise as N


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def residuals(z, cbs, idx, level):
    """fp32 [N, D]: the residual entering ``level`` -- z minus the chosen codewords of the levels below, one fp32 subtraction per level."""
    r = np.array(z, dtype=np.float32)
    for l in range(level):
        r = r - np.asarray(cbs[l], dtype=np.float32)[idx[:, l]]
    return r


def fix_unit(z, cbs, last):
    """2^(e-39): the bound on one conversion's error when levels up to ``last`` are walked."""
    m = float(np.abs(z).max()) + sum(float(np.abs(cbs[l]).max()) for l in range(last))
    e = int(np.frexp(m)[1]) if m > 0 else 0
    return 2.0 ** (e - 39)


def sure(r, means, rel=1e-5):
    """(fp64 indices, mask of the rows whose best and next fp64 distances differ by at least ``rel`` relative)."""
    i, best, nxt = N.codebook_assign(r, means)
    return i, (nxt - best) / nxt >= rel


def train_step(z, cbs, cs, avg, idx, decay, commitment_weight, threshold, seed, draw_index):
    """One training step of every level from the given (the device's) indices [N, L].  Returns per level a dict: cs / avg / embed before
    expiry (fp32-rounded as the device stores them), cs2 / avg2 / embed2 after it, dead (indices of the replaced codes), counts, loss
    (fp64), and the tolerances tol_avg / tol_embed / tol_loss = one fp32 ulp of the value + the accumulation bound carried through."""
    n, d = z.shape
    levels, k = cbs.shape[0], cbs.shape[1]
    unit, om, out = fix_unit(z, cbs, levels - 1), 1.0 - float(decay), []
    for l in range(levels):
        r = residuals(z, cbs, idx, l)
        counts, sums = N.codebook_sums(r, idx[:, l], k)
        commit = float(((r.astype(np.float64) - cbs[l].astype(np.float64)[idx[:, l]]) ** 2).sum())
        c, a, e = N.codebook_ema(cs[l], avg[l], counts, sums, decay)
        c64 = c.astype(np.float64)
        tot = float(np.cumsum(c64)[-1])
        smoothed = (c64 + N.CODEBOOK_EPS) / (tot + k * N.CODEBOOK_EPS) * tot
        tol_avg = ulp32(a) + om * counts[:, None] * unit
        tol_embed = ulp32(e) + tol_avg / smoothed[:, None] * (1 + 2.0 ** -20)
        loss = commitment_weight * commit / (n * d)
        c2, a2, e2, dead = N.codebook_expire(c, a, e, r, threshold, seed, l, draw_index)
        out.append(dict(cs=c, avg=a, embed=e, cs2=c2, avg2=a2, embed2=e2, dead=dead, counts=counts, loss=loss, tol_avg=tol_avg,
                        tol_embed=tol_embed, tol_loss=float(ulp32(loss)) + loss * n * d * 2.0 ** -52))
    return out


def lloyd_update(r, means, idx):
    """One Lloyd update of fp32 means from given indices: (means fp64 with empty clusters kept, counts, objective)."""
    k = len(means)
    counts, sums = N.codebook_sums(r, idx, k)
    new = np.array(means, dtype=np.float64)
    full = counts > 0
    new[full] = sums[full] / counts[full, None]
    obj = float(((np.asarray(r, dtype=np.float64) - np.asarray(means, dtype=np.float64)[idx]) ** 2).sum())
    return new, counts, obj
