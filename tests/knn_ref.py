"""fp64 NumPy restatement of flocoder_amd.neighbors and metrics.prdc (test infrastructure; the product never imports it).

d2 is formed by direct differences in float64; a non-finite d2, or one beyond FLT_MAX, counts as FLT_MAX, as the library stores it.
Neighbours are ordered by (d2, global reference index) lexicographically: a stable sort over references in index order."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)


def pairwise_d2(q, r):
    """[Q, N] float64 squared distances of the flattened rows, direct differences, non-finite / overflowing entries -> FLT_MAX."""
    q = np.asarray(q, dtype=np.float64).reshape(len(q), -1)
    r = np.asarray(r, dtype=np.float64).reshape(len(r), -1)
    out = np.empty((q.shape[0], r.shape[0]), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(q.shape[0]):
            diff = r - q[i]
            out[i] = np.einsum("nf,nf->n", diff, diff)
    out[~(out <= FLT_MAX)] = FLT_MAX                      # NaN and +inf fail the comparison
    return out


def knn_ref(q, r, k, query_ids=None, first_index=0, d2=None):
    """(d2 [Q,k] float64, idx [Q,k] int64): the k smallest (d2, first_index + row) per query, ascending; reference `query_ids[q]` is left
    out for query q; missing slots are (+inf, -1).  `d2` may pass a precomputed pairwise matrix."""
    d2 = pairwise_d2(q, r) if d2 is None else d2
    nq, n = d2.shape
    out_d = np.full((nq, k), np.inf, dtype=np.float64)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    gidx = first_index + np.arange(n, dtype=np.int64)
    for i in range(nq):
        keep = np.ones(n, dtype=bool) if query_ids is None else gidx != int(query_ids[i])
        order = np.argsort(d2[i][keep], kind="stable")[:k]
        out_d[i, :len(order)] = d2[i][keep][order]
        out_i[i, :len(order)] = gidx[keep][order]
    return out_d, out_i


def ball_counts_ref(q, r, radius2, query_ids=None, first_index=0, d2=None):
    """int64 [Q]: per query #{r: d2(q, r) <= radius2[r]} (reference `query_ids[q]` left out)."""
    d2 = pairwise_d2(q, r) if d2 is None else d2
    inside = d2 <= np.asarray(radius2, dtype=np.float64).reshape(1, -1)
    if query_ids is not None:
        gidx = first_index + np.arange(d2.shape[1], dtype=np.int64)
        inside &= gidx[None, :] != np.asarray(query_ids, dtype=np.int64)[:, None]
    return inside.sum(axis=1).astype(np.int64)


def prdc_ref(real, fake, k):
    """The four numbers of metrics.prdc from their definitions on squared distances."""
    n, m = len(real), len(fake)
    d_rr, d_ff, d_rf = pairwise_d2(real, real), pairwise_d2(fake, fake), pairwise_d2(real, fake)
    r_real = knn_ref(real, real, k, query_ids=np.arange(n), d2=d_rr)[0][:, k - 1]
    r_fake = knn_ref(fake, fake, k, query_ids=np.arange(m), d2=d_ff)[0][:, k - 1]
    in_real = (d_rf <= r_real[:, None])                      # [i, j]: fake j lies in real i's ball
    in_fake = (d_rf <= r_fake[None, :])                      # [i, j]: real i lies in fake j's ball
    return {"precision": float(in_real.any(axis=0).sum()) / m, "recall": float(in_fake.any(axis=1).sum()) / n,
            "density": float(in_real.sum()) / (k * m), "coverage": float((d_rf.min(axis=1) <= r_real).sum()) / n}


def error_bound(dim):
    """Relative bound on the fp32 d2 of `dim` features against the exact one, for any summation order: a term (a - b)^2 carries the
    difference's rounding twice ((1 + u)^2; the square itself is not rounded inside an fma) and then at most `dim` roundings of the
    accumulations it takes part in; all terms are non-negative, so the sum's relative error is at most the largest factor's,
    (1 + u)^(dim + 2) - 1 <= gamma_{dim+2} = (dim + 2) u / (1 - (dim + 2) u), u = 2^-24."""
    u = 2.0 ** -24
    return (dim + 2) * u / (1.0 - (dim + 2) * u)


def grid_points(rng, n, dim):
    """Integer-valued fp32 rows whose every partial sum of squared differences is exact in fp32 under any order: coordinates in
    {-1, 0, 1} up to 16 features, {-3..3} above, so dim * (2 max)^2 < 2^24 for every dim the tests use."""
    hi = 1 if dim <= 16 else 3
    assert dim * (2 * hi) ** 2 < 2 ** 24
    return rng.integers(-hi, hi + 1, size=(n, dim)).astype(np.float32)


# ---- the shapes and inputs the CPU and GPU tests share -----------------------------------------------------------------------------
QS, NS, DS, KS = (1, 3, 65), (1, 4, 63, 65, 200), (1, 3, 4, 36, 260), (1, 5, 64)
RADIUS_K = 5                                                  # ball radii: a reference's 5th neighbour among the other references


def case_seed(nq, n, dim):
    return 1000003 * nq + 1009 * n + dim


def exact_case(nq, n, dim):
    """(queries [nq, dim], refs [n, dim]) on the integer grid: duplicates and ties everywhere at small dim."""
    rng = np.random.default_rng(case_seed(nq, n, dim))
    return grid_points(rng, nq, dim), grid_points(rng, n, dim)


def gauss_case(nq, n, dim):
    rng = np.random.default_rng(case_seed(nq, n, dim) + 1)
    return rng.standard_normal((nq, dim)).astype(np.float32), rng.standard_normal((n, dim)).astype(np.float32)


def radii(refs):
    """fp32 [N]: each reference's squared distance to its RADIUS_K-th neighbour among the others (the last one there is when there are
    fewer; its own squared norm when it is alone) -- PRDC's radii."""
    n = len(refs)
    if n == 1:
        return (np.asarray(refs, dtype=np.float64) ** 2).sum(axis=1).astype(np.float32)
    kk = min(RADIUS_K, n - 1)
    return knn_ref(refs, refs, kk, query_ids=np.arange(n))[0][:, kk - 1].astype(np.float32)
