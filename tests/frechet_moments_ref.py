"""fp64 restatement of the moment form of the Frechet distance (flocoder_amd.distances.FrechetMoments / frechet_distance_moments,
csrc/frechet.hip): Chan's pairwise update of (n, mean, M), the factor F with F^T F = S from the Jacobi iteration in the device's
schedule run on S itself, the distance, and the error bound of DESIGN.md section 4 "Set distances -- the moment form".  The Jacobi
schedule, the LAPACK form, the sample form's bounds and the case generators are tests/frechet_ref.py's."""
import math

import numpy as np

import frechet_ref as R

U, MAX_SWEEPS = R.U, R.MAX_SWEEPS


# ---- the state -------------------------------------------------------------------------------------------------------------------------
class Moments:
    """n, mean [D], M [D, D] = sum (x - mean)(x - mean)^T; `batches` counts the updates and merges that built it (the bound wants it)."""

    def __init__(self):
        self.n, self.mean, self.M, self.batches = 0, None, None, 0

    def update(self, xb):
        xb = R.rows(xb).astype(np.float64)
        mb = xb.mean(axis=0)
        c = xb - mb
        return self._join(len(xb), mb, c.T @ c, 1)

    def merge(self, other):
        return self._join(other.n, other.mean, other.M, other.batches)

    def _join(self, nb, mb, sb, batches):
        if self.n == 0:
            self.n, self.mean, self.M = nb, mb.copy(), sb.copy()
        else:
            d = mb - self.mean
            tot = float(self.n + nb)
            self.M = self.M + (sb + (self.n * nb / tot) * np.outer(d, d))
            self.mean = self.mean + (nb / tot) * d
            self.n += nb
        self.batches += batches
        return self

    def covariance(self):
        return self.M / (self.n - 1)


def moments_of(x, splits=None):
    """The state after feeding x in batches of `splits` rows (None: one batch)."""
    st, r0 = Moments(), 0
    for nb in (splits or (len(x),)):
        st.update(x[r0:r0 + nb])
        r0 += nb
    assert r0 == len(x)
    return st


def raw_covariance(x):
    """What metrics.FrechetStatistics keeps: (ss - n mu mu^T) / (n - 1) from the raw fp64 sums."""
    x = R.rows(x).astype(np.float64)
    n, mu = len(x), x.sum(axis=0) / len(x)
    return (x.T @ x - n * np.outer(mu, mu)) / (n - 1)


def exact_covariance(x):
    """The covariance of the fp32 rows computed in longdouble (11 more bits than the forms under test) and rounded once."""
    x = R.rows(x).astype(np.longdouble)
    c = x - x.mean(axis=0)
    return np.asarray((c.T @ c) / (len(x) - 1), dtype=np.float64)


# ---- the factor ------------------------------------------------------------------------------------------------------------------------
def jacobi_rows(mat):
    """frechet_ref.jacobi_svals, returning the rotated rows as well: (z, row norms squared, sweeps, converged)."""
    z = np.array(mat, dtype=np.float64)
    n, r = z.shape
    m = n + (n & 1)
    fl = (U * float((z * z).sum())) ** 2
    tol = r * U
    sweeps, conv = 0, False
    for sweeps in range(1, MAX_SWEEPS + 1):
        rotations = 0
        for rnd in range(m - 1):
            ia, ib = R.round_pairs(m, rnd)
            keep = ib < n
            ia, ib = ia[keep], ib[keep]
            a, b = z[ia], z[ib]
            al, be, ga = (a * a).sum(axis=1), (b * b).sum(axis=1), (a * b).sum(axis=1)
            if not (np.isfinite(al).all() and np.isfinite(be).all() and np.isfinite(ga).all()):
                return z, (z * z).sum(axis=1), sweeps, False
            rot = (np.abs(ga) > tol * np.sqrt(al * be)) & (al * be > fl)
            if not rot.any():
                continue
            ia, ib, a, b, al, be, ga = ia[rot], ib[rot], a[rot], b[rot], al[rot], be[rot], ga[rot]
            zeta = (be - al) / (2.0 * ga)
            t = np.copysign(1.0, zeta) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
            c = 1.0 / np.sqrt(1.0 + t * t)
            s = c * t
            z[ia], z[ib] = c[:, None] * a - s[:, None] * b, s[:, None] * a + c[:, None] * b
            rotations += int(rot.sum())
        if rotations == 0:
            conv = True
            break
    return z, (z * z).sum(axis=1), sweeps, conv


def factor(s):
    """(F, eigenvalues descending, sweeps, converged): the rows of the symmetric PSD `s` rotated until orthogonal are z_i = lambda_i v_i^T;
    f_i = z_i / sqrt(|z_i|) (zero rows stay zero), so F^T F = sum lambda_i v_i v_i^T = s."""
    z, alpha, sweeps, conv = jacobi_rows(s)
    scale = np.zeros_like(alpha)
    ok = alpha > 0.0
    scale[ok] = 1.0 / np.sqrt(np.sqrt(alpha[ok]))
    return z * scale[:, None], np.sort(np.sqrt(alpha))[::-1], sweeps, conv


def frechet_moments(a, b):
    """(FD, info) from two Moments: |ma - mb|^2 + tr Sa + tr Sb - 2 ||Fa Fb^T||_*."""
    sa, sb = a.covariance(), b.covariance()
    fa, eva, swa, ca = factor(sa)
    fb, evb, swb, cb = factor(sb)
    sv, swp, cp = R.jacobi_svals(fa @ fb.T)
    dm2, ta, tb = float(((a.mean - b.mean) ** 2).sum()), float(np.trace(sa)), float(np.trace(sb))
    return dm2 + ta + tb - 2.0 * float(sv.sum()), {"sweeps": (swa, swb, swp), "converged": ca and cb and cp, "evals": (eva, evb), "svals": sv}


# ---- the bound (DESIGN.md section 4 "Set distances -- the moment form") -------------------------------------------------------------------
def set_scalars(x):
    """(n, D, tr S, max row norm A) of a sample set: what the scatter term is written in."""
    x = R.rows(x).astype(np.float64)
    c = x - x.mean(axis=0)
    return len(x), x.shape[1], float((c * c).sum() / (len(x) - 1)), float(np.sqrt((x * x).sum(axis=1).max()))


def mean_term(n, batches, amax):
    """|computed mean - mean| <= (n + 4 k + 1) u A: a batch mean of nb <= n fp32 values per feature sums to within nb u of its mean
    absolute value and divides once; every join forms the convex combination mean + (nb / N) d of two such means in three roundings of
    quantities no larger than 2 A, and a convex combination of errors is no larger than the larger one."""
    return (n + 4 * batches + 1) * U * amax


def scatter_term(n, dim, batches, trs, amax):
    """||S_computed - S||_F for k = `batches` joins, first order in u:
      (n + 2) u tr S                 each batch scatter entry is an fp64 inner product of nb <= n centred values (two more roundings for
                                     the centring), any order: |error| <= (nb + 2) u sum_r |c_rf| |c_rg|, whose Frobenius norm over (f, g)
                                     is at most (nb + 2) u tr M_b by Cauchy-Schwarz; sum_b tr M_b <= tr M.  (An error e_b of the batch mean
                                     used for the centring adds nb e_b e_b^T: second order.)
      (2 k + 5) u tr S               two additions per join into partial sums that are PSD, so of Frobenius norm <= tr M; the three
                                     roundings of w d d^T, sum_b w_b |d_b|^2 <= tr M.
      4 (n + 4 k + 1) u A sqrt(n tr S / (n - 1))
                                     d is formed from two computed means, each within mean_term of its own: w (d e^T + e d^T) has norm
                                     2 w |d| |e|, |e| <= 2 mean_term, and sum_b w_b |d_b| <= sqrt(sum w_b) sqrt(sum w_b |d_b|^2)
                                     <= sqrt(n tr M) since w_b <= nb."""
    return U * ((n + 2 * batches + 7) * trs + 4.0 * (n + 4 * batches + 1) * amax * math.sqrt(n * trs / (n - 1.0)))


def factor_term(dim, fro, lam_max, evals):
    """||F^T F - S_computed||_F.  The iteration leaves Z = Q (S + E) with Q orthogonal, ||E||_F <= 8 u SWEEPS (D - 1) ||S||_F (the rotation
    term of svals_bound, as a matrix), and Z = diag(|z_i|) W with unit rows, |w_i . w_j| <= D u off the floor (the stopping rule), so
    ||W - W0||_F <= D^2 u for the nearest orthogonal W0.  F^T F = W^T diag(|z_i|) W, and W0^T diag W0 is exactly the PSD square root of
    B^T B for B = Q^T diag W0, which is within lam_max D^2 u of S + E.  The PSD polar factor moves by at most sqrt(2) times the
    matrix (Frobenius), S = sqrt(S^T S), and replacing W0 by W costs 2 lam_max D^2 u:
         sqrt(2) 8 u SWEEPS (D - 1) ||S||_F + (2 + sqrt(2)) D^2 u lam_max + 16 u ||S||_F  (the scaling's roundings)
    plus the floor: a row under the floor (norm^2 <= 2 u ||S||_F^2) may not be orthogonal to the others; taking it out moves Z by its norm
    and F^T F by its norm: (1 + sqrt(2)) floor_term."""
    return (math.sqrt(2.0) * 8.0 * U * MAX_SWEEPS * (dim - 1) * fro + (2.0 + math.sqrt(2.0)) * dim * dim * U * lam_max + 16.0 * U * fro
            + (1.0 + math.sqrt(2.0)) * R.floor_term(evals, fro))


def sqrt_term(dim, eps, lam_min):
    """||sqrt(S') - sqrt(S)||_F for PSD S, S' with ||S' - S||_F <= eps.  Above the smallest eigenvalue the square root is Lipschitz:
    eps / (sqrt(lmin(S')) + sqrt(lmin(S))), with both lmin >= lam_min - 2 eps for the returned smallest eigenvalue lam_min (Weyl).  For
    eigenvalues under that noise floor there is no such constant and only the floor remains: the Powers-Stormer inequality
    ||sqrt(S') - sqrt(S)||_F^2 <= ||S' - S||_* <= sqrt(D) eps.  The smaller of the two holds."""
    floor = math.sqrt(math.sqrt(dim) * eps)
    low = lam_min - 2.0 * eps
    return min(eps / (2.0 * math.sqrt(low)), floor) if low > 0.0 else floor


def moments_bound_parts(x, y, batches=(1, 1), evals=None, svals=None):
    """The four parts of |FD_moments - FD_lapack| and the pieces the tests assert on their own.  `evals`: the returned eigenvalues of both
    covariances, `svals`: the returned singular values of F1 F2^T (None: the restatement's)."""
    sets = [set_scalars(v) for v in (x, y)]
    dim = sets[0][1]
    cov = [exact_covariance(v) for v in (x, y)]
    if evals is None or svals is None:
        fa, eva = factor(cov[0])[:2]
        fb, evb = factor(cov[1])[:2]
        evals = (eva, evb) if evals is None else evals
        svals = R.jacobi_svals(fa @ fb.T)[0] if svals is None else svals
    eps, root, scat, fact, means = [], [], [], [], []
    for (n, _, trs, amax), k, s, ev in zip(sets, batches, cov, evals):
        ev = np.asarray(ev, dtype=np.float64)
        fro = float(np.linalg.norm(s))
        scat.append(scatter_term(n, dim, k, trs, amax))
        fact.append(factor_term(dim, fro, float(ev.max()), ev))
        eps.append(scat[-1] + fact[-1])
        root.append(sqrt_term(dim, eps[-1], float(ev.min())))
        means.append(mean_term(n, k, amax))
    (n1, _, t1, _), (n2, _, t2, _) = sets
    dm2 = float(((R.rows(x).astype(np.float64).mean(axis=0) - R.rows(y).astype(np.float64).mean(axis=0)) ** 2).sum())
    # tr sqrt(S1 S2) = ||sqrt(S1) sqrt(S2)||_*, ||X Y||_* <= ||X||_F ||Y||_F, ||sqrt(S)||_F^2 = tr S
    perturb = root[0] * math.sqrt(t2 + math.sqrt(dim) * eps[1]) + math.sqrt(t1) * root[1]
    svals = np.asarray(svals, dtype=np.float64)
    g_fro, nuc = float(np.sqrt((svals * svals).sum())), float(svals.sum())
    product = R.nuclear_bound(dim, dim, g_fro, nuc, svals) + math.sqrt(dim) * (dim + 2) * U * math.sqrt(t1 * t2)   # the Jacobi solve + the fp64 Gram
    # the traces (a diagonal's sum: sqrt(D) ||E||_F and D u tr S), the mean term, the three additions; then the reference's own Gram and sums
    plain = (math.sqrt(dim) * (scat[0] + scat[1]) + (dim + 8) * U * (dm2 + t1 + t2) + 2.0 * math.sqrt(dm2) * (means[0] + means[1])
             + (means[0] + means[1]) ** 2)
    ns, nl = min(n1, n2), max(n1, n2)
    reference = 2.0 * R.gram_term(ns, nl, dim, t1, t2) + (nl + dim + 8) * U * (dm2 + t1 + t2)
    return {"scatter": scat, "factor": fact, "eps": eps, "sqrt": root, "perturb": perturb, "product": product, "plain": plain,
            "reference": reference, "total": 2.0 * (perturb + product) + plain + reference}


def moments_bound(x, y, batches=(1, 1), evals=None, svals=None):
    return moments_bound_parts(x, y, batches, evals, svals)["total"]


def eigenvalue_bound(n, dim, batches, trs, amax, fro, lam, got):
    """Per eigenvalue against eigvalsh of an fp64 covariance of the same rows: both covariances are within their scatter terms of the
    exact one (Weyl), and the returned values are the singular values of the computed S inside svals_bound."""
    return scatter_term(n, dim, batches, trs, amax) + scatter_term(n, dim, 1, trs, amax) + R.svals_bound(dim, dim, fro, lam, got)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
SPLITS = (17, 130, 1, 152)


def uneven(n):
    """An uneven split of n rows that has a single-row batch in it."""
    head = (17, 1, 31) if n >= 100 else (7, 1)
    return head + (n - sum(head),)


def shifted(sets, by=100.0):
    """Every feature + `by` (fp32, as the device reads it)."""
    return tuple((np.asarray(v) + np.float32(by)).astype(np.float32) for v in sets)
