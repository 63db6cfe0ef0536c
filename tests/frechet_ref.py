"""fp64 restatement of flocoder_amd.distances (csrc/frechet.hip): the definitions, the Jacobi iteration in the device's schedule, the
LAPACK form, the error bounds of DESIGN.md section 4 "Set distances", and the case generators the CPU and GPU tests share."""
import functools
import math

import numpy as np

U = 2.0 ** -53
MAX_SWEEPS = 30


# ---- definitions ---------------------------------------------------------------------------------------------------------------------
def rows(x):
    return np.asarray(x).reshape(len(x), -1)


def gram64(a, b, center=False):
    """sum_f (a_if - ma_f)(b_jf - mb_f) in fp64 from the fp32 rows; the means are the fp64 column means."""
    a, b = rows(a).astype(np.float64), rows(b).astype(np.float64)
    if center:
        a, b = a - a.mean(axis=0), b - b.mean(axis=0)
    return a @ b.T


def frechet_parts(x, y):
    """(|mx - my|^2, tr S1, tr S2, C) with C the centred cross-Gram of the smaller set against the larger, scaled by
    1 / sqrt((N1 - 1)(N2 - 1)): FD = dm2 + t1 + t2 - 2 ||C||_*."""
    x, y = rows(x).astype(np.float64), rows(y).astype(np.float64)
    n1, n2 = len(x), len(y)
    mx, my = x.mean(axis=0), y.mean(axis=0)
    xc, yc = x - mx, y - my
    a, b = (xc, yc) if n1 <= n2 else (yc, xc)
    c = (a @ b.T) / math.sqrt((n1 - 1.0) * (n2 - 1.0))
    return float(((mx - my) ** 2).sum()), float((xc ** 2).sum() / (n1 - 1)), float((yc ** 2).sum() / (n2 - 1)), c


def frechet_lapack(x, y):
    """The LAPACK form: np.linalg.svd of the fp64 Gram of the same fp32 inputs."""
    dm2, t1, t2, c = frechet_parts(x, y)
    return dm2 + t1 + t2 - 2.0 * float(np.linalg.svd(c, compute_uv=False).sum())


def frechet_jacobi(x, y):
    """The same with the restated Jacobi iteration: (FD, sweeps, converged)."""
    dm2, t1, t2, c = frechet_parts(x, y)
    sv, sweeps, conv = jacobi_svals(c)
    return dm2 + t1 + t2 - 2.0 * float(sv.sum()), sweeps, conv


def kid_sums(x, y):
    x, y = rows(x).astype(np.float64), rows(y).astype(np.float64)
    d = x.shape[1]
    kxx, kyy, kxy = ((x @ x.T) / d + 1.0) ** 3, ((y @ y.T) / d + 1.0) ** 3, ((x @ y.T) / d + 1.0) ** 3
    return float(kxx.sum() - np.trace(kxx)), float(kyy.sum() - np.trace(kyy)), float(kxy.sum())


def kid_ref(x, y):
    """Unbiased MMD^2 with k(x, y) = (x.y / D + 1)^3 over all pairs."""
    n1, n2 = len(x), len(y)
    sxx, syy, sxy = kid_sums(x, y)
    return sxx / (n1 * (n1 - 1.0)) + syy / (n2 * (n2 - 1.0)) - 2.0 * sxy / (n1 * float(n2))


# ---- one-sided Jacobi in the device's schedule -------------------------------------------------------------------------------------------
def round_pairs(m, rnd):
    """Round `rnd` (0 .. m - 2) of the circle schedule on m (even) players: (m - 1, rnd) and (rnd + p, rnd - p) mod (m - 1)."""
    p = np.arange(1, m // 2)
    ia = np.concatenate([[m - 1], (rnd + p) % (m - 1)])
    ib = np.concatenate([[rnd], (rnd - p) % (m - 1)])
    return np.minimum(ia, ib), np.maximum(ia, ib)


def jacobi_svals(mat, floor=True):
    """Singular values (descending) of `mat` [n, r] by rotating its rows: (svals, sweeps, converged)."""
    z = np.array(mat, dtype=np.float64)
    n, r = z.shape
    m = n + (n & 1)
    fl = (U * float((z * z).sum())) ** 2 if floor else -1.0
    tol = r * U
    sweeps, conv = 0, False
    for sweeps in range(1, MAX_SWEEPS + 1):
        rotations = 0
        for rnd in range(m - 1):
            ia, ib = round_pairs(m, rnd)
            keep = ib < n                                        # the padding vector's pair has nothing to do
            ia, ib = ia[keep], ib[keep]
            a, b = z[ia], z[ib]
            al, be, ga = (a * a).sum(axis=1), (b * b).sum(axis=1), (a * b).sum(axis=1)
            if not (np.isfinite(al).all() and np.isfinite(be).all() and np.isfinite(ga).all()):
                return np.sort(np.sqrt((z * z).sum(axis=1)))[::-1], sweeps, False
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
    return np.sort(np.sqrt((z * z).sum(axis=1)))[::-1], sweeps, conv


# ---- bounds (DESIGN.md section 4 "Set distances") --------------------------------------------------------------------------------------
def floor_term(svals, fro):
    """The part of the bound the noise floor owns: pairs with alpha beta <= (u F^2)^2 are never rotated, and such a pair has a member
    with alpha <= u F^2.  Removing those vectors lowers no singular value by more than their joint norm and the nuclear norm by no
    more than the sum of their norms; the returned norms of that size (with a factor 2 for the rounding of the norms) are summed."""
    sv = np.asarray(svals, dtype=np.float64)
    return float(sv[sv * sv <= 2.0 * U * fro * fro].sum())


def svals_bound(n, r, fro, sigma, svals):
    """|sigma_i - computed_i| <= 8 u S (n - 1) F  [rounding of at most S (n - 1) rotations per vector, 8 u each, Mirsky]
                                 + n r u sigma_i   [stopping rule |gamma| <= r u sqrt(alpha beta): Ostrowski, (n - 1) r u / 2 and slack]
                                 + the floor term."""
    return 8.0 * U * MAX_SWEEPS * (n - 1) * fro + n * r * U * np.asarray(sigma) + floor_term(svals, fro)


def nuclear_bound(n, r, fro, nuclear, svals):
    """The same summed: sqrt(n) times the rotation term (Mirsky, Cauchy-Schwarz), the relative term on the sum, the floor term once."""
    return 8.0 * U * MAX_SWEEPS * (n - 1) * math.sqrt(n) * fro + n * r * U * nuclear + floor_term(svals, fro)


def gram_term(ns, nl, dim, t1, t2):
    """What the rounding of an fp64 Gram of fp32 rows (any summation order, centring included) can move ||C||_*:
    ||E||_* <= sqrt(ns) ||E||_F <= sqrt(ns) (dim + nl + 4) u sqrt(tr S1 tr S2)."""
    return math.sqrt(ns) * (dim + nl + 4) * U * math.sqrt(t1 * t2)


def frechet_bound(x, y, svals=None):
    """|FD_device - FD_lapack| <= 2 (Jacobi bound on ||C||_* + the Gram term of both sides) + the rounding of the three plain sums.
    `svals`: the device's singular values (for the floor term); None: the restatement's."""
    n1, n2 = len(x), len(y)
    ns, nl, dim = min(n1, n2), max(n1, n2), rows(x).shape[1]
    dm2, t1, t2, c = frechet_parts(x, y)
    sv = jacobi_svals(c)[0] if svals is None else np.asarray(svals)
    fro, nuc = float(np.linalg.norm(c)), float(np.linalg.svd(c, compute_uv=False).sum())
    plain = (nl + dim + 8) * U * (dm2 + t1 + t2)
    return 2.0 * (nuclear_bound(ns, nl, fro, nuc, sv) + 2.0 * gram_term(ns, nl, dim, t1, t2)) + 2.0 * plain


def kid_bound(x, y):
    """|MMD^2_device - MMD^2_fp64| for any summation order on both sides: with s = max |x_i| |y_j| and K = (s / D + 1)^3 every term is at
    most K in size, a term's own error is at most 3 (D + 8) u K (the dot product's (D + 2) u s / D <= (D + 2) u (s / D + 1), cubed) and a
    sum of T terms adds at most T u K per term; the three means are combined with weights 1, 1, 2, and both sides err: a factor 2."""
    x, y = rows(x).astype(np.float64), rows(y).astype(np.float64)
    d = x.shape[1]
    s = max(float((x * x).sum(axis=1).max()), float((y * y).sum(axis=1).max()))
    k = (s / d + 1.0) ** 3
    terms = max(len(x), len(y)) ** 2
    return 2.0 * 4.0 * k * U * (terms + 3.0 * (d + 8))


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_case(n1, n2, dim, seed=0):
    """Small integers (|v| <= 3): every product and partial sum is an exact fp64 integer under any order."""
    rng = np.random.default_rng(1000 * n1 + 10 * n2 + dim + seed)
    a, b = rng.integers(-3, 4, size=(n1, dim)).astype(np.float32), rng.integers(-3, 4, size=(n2, dim)).astype(np.float32)
    a.setflags(write=False), b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def dyadic_mean_case(n1, n2, dim, seed=0):
    """exact_case with every column mean an integer: row 0 is moved so that each column sums to 0, then column f is shifted by the
    integer (f mod 5) - 2, its mean (|v| <= 3 n + 2).  Means and centred values are integers and the centred Gram is exact as well."""
    out = []
    for arr in exact_case(n1, n2, dim, seed):
        arr = arr.copy()
        arr[0] -= arr.sum(axis=0)
        arr += (np.arange(dim) % 5 - 2).astype(np.float32)
        arr.setflags(write=False)
        out.append(arr)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def gauss_sets(n1, n2, dim, shift=0.25, seed=0):
    rng = np.random.default_rng(7000 + 100 * n1 + 10 * n2 + dim + seed)
    x = rng.standard_normal((n1, dim)).astype(np.float32)
    y = (rng.standard_normal((n2, dim)) * 1.1 + shift).astype(np.float32)
    x.setflags(write=False), y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def near_identical_sets(n=64, dim=128, noise=1e-3, seed=0):
    rng = np.random.default_rng(42 + seed)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    y = (x + noise * rng.standard_normal((n, dim))).astype(np.float32) if noise else x.copy()
    x.setflags(write=False), y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def gauss_matrix(n, r, rank=None, seed=0):
    """Gaussian [n, r] fp64, of rank `rank` (a product of two Gaussian factors) when given."""
    rng = np.random.default_rng(300 + 17 * n + r + seed)
    m = rng.standard_normal((n, r)) if rank is None else rng.standard_normal((n, rank)) @ rng.standard_normal((rank, r))
    m.setflags(write=False)
    return m


JACOBI_CASES = ((2, 2, None), (5, 7, None), (48, 64, 31), (96, 96, None), (128, 128, 63))
FRECHET_SHAPES = ((63, 65, 36), (130, 17, 260), (2, 2, 1))
