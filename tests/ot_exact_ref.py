"""NumPy fp64 restatement of the exact OT pairing's assignment solver (csrc/ot.hip, ot_assign_kernel), the optimality certificate
the tests hold it to, and the cost matrices those tests use (shared by the CPU and the GPU tests: same generators, same seeds).

The solver, as in the kernel: non-finite entries count as FLT_MAX; start u_i = min_j c_ij, v = 0, row i takes its first-minimum column
if no earlier row has it; then, for every free row in ascending order, a Dijkstra over columns on the reduced costs
path + ((c_ij - u_i) - v_j), `<` keeps the first predecessor, the nearest unvisited column is the first minimum, until that column is
free; the duals move by (radius - minv_j) on the visited columns with minv_j < radius and their rows, radius being the last path
length below FLT_MAX / 2 (the whole path unless a finite row was driven onto a sentinel), the path's matches flip.  Every loop is
bounded by B.

The certificate (weak duality): with c the fp32 matrix in fp64 arithmetic, phi = max(0, max_ij(u_i + v_j - c_ij)) and
g = sum_i c[i, perm[i]] - sum u - sum v, any permutation costs at least sum u + sum v - B phi, so cost(perm) - OPT <= g + B phi.
The bound tau = B^3 2^-52 max(c): each of the 2B duals is the result of at most B^2 fp64 additions of magnitude <= max(c).  g is summed
pair by pair, and the duals must be of the costs' scale, max(|u|, |v|) <= (2 B^2 + 1) max|c| (at most B augmentations, each moving a dual
by at most a path of B reduced costs of at most 2 max|c|, on top of a start value of at most max|c|): duals of a larger scale absorb
the costs in fp64 and would make g and phi vanish whatever the pairing.  max(c) and max|c| range over the non-sentinel entries."""
import itertools

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
BIG = 0.5 * FLT_MAX                                   # OT_BIG in csrc/ot.hip


def clean(cost):
    """The matrix as the solver reads it: fp32, NaN and +-inf replaced by FLT_MAX."""
    c = np.asarray(cost, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(c) <= np.float32(FLT_MAX), c, np.float32(FLT_MAX)).astype(np.float32)


def assign(cost, stats=None):
    """(perm int64 [B], u fp64 [B], v fp64 [B]) of the B x B matrix ``cost``.  ``stats``: a dict that receives the visit count."""
    c = clean(cost).astype(np.float64)
    n = c.shape[0]
    assert c.shape == (n, n) and n >= 1
    u = c.min(1)
    v = np.zeros(n)
    col4row = np.full(n, -1, dtype=np.int64)
    row4col = np.full(n, -1, dtype=np.int64)
    for i in range(n):
        j = int(np.argmin(c[i]))                      # first minimum
        if row4col[j] < 0:
            row4col[j], col4row[i] = i, j
    visits = augmentations = 0
    for cur in range(n):
        if col4row[cur] >= 0:
            continue
        augmentations += 1
        minv = np.full(n, np.inf)
        way = np.full(n, -1, dtype=np.int64)
        vis = np.zeros(n, dtype=bool)
        i, sink, path, radius = cur, -1, 0.0, 0.0
        for _ in range(n):
            visits += 1
            r = path + ((c[i] - u[i]) - v)           # c - u first: exact (zero) on a row of sentinels, whatever the path
            upd = ~vis & (r < minv)
            minv[upd] = r[upd]
            way[upd] = i
            cand = np.where(vis, np.inf, minv)
            bj = int(np.argmin(cand))                 # first minimum among the unvisited
            path = float(cand[bj])
            if path < BIG:
                radius = path                         # the dual update stops before a hop of sentinel scale
            vis[bj] = True
            if row4col[bj] < 0:
                sink = bj
                break
            i = int(row4col[bj])
        assert sink >= 0
        inside = vis & (radius - minv > 0.0)
        d = radius - minv[inside]
        v[inside] -= d
        rows = row4col[inside]
        u[rows[rows >= 0]] += d[rows >= 0]
        u[cur] += radius
        j = sink
        for _ in range(n):
            r = int(way[j])
            row4col[j] = r
            col4row[r], j = j, int(col4row[r])
            if r == cur:
                break
    if stats is not None:
        stats.update(visits=visits, augmentations=augmentations)
    return col4row, u, v


def perm_cost(cost, perm):
    c = clean(cost).astype(np.float64)
    return float(c[np.arange(c.shape[0]), np.asarray(perm)].sum())


def brute_force(cost):
    """The optimal cost by enumeration (B <= 7)."""
    c = clean(cost).astype(np.float64)
    n = c.shape[0]
    rows = np.arange(n)
    return min(float(c[rows, list(p)].sum()) for p in itertools.permutations(range(n)))


def certificate(cost, perm, u, v):
    """(g + B phi, tau) on the fp32 matrix ``cost`` in fp64 arithmetic."""
    c = clean(cost).astype(np.float64)
    n = c.shape[0]
    u, v, perm = np.asarray(u, np.float64), np.asarray(v, np.float64), np.asarray(perm)
    real = c[c < FLT_MAX]
    cmax, cabs = (float(real.max()), float(np.abs(real).max())) if real.size else (FLT_MAX, FLT_MAX)
    if max(float(np.abs(u).max()), float(np.abs(v).max())) > (2 * n * n + 1) * cabs:
        return float("inf"), n ** 3 * 2.0 ** -52 * cmax          # duals out of the costs' scale certify nothing
    phi = max(0.0, float((u[:, None] + v[None, :] - c).max()))
    g = float(((c[np.arange(n), perm] - u) - v[perm]).sum())
    return g + n * phi, n ** 3 * 2.0 ** -52 * cmax


def finite_part(cost, perm, u, v):
    """Drop the rows matched to a sentinel entry together with their columns: (sub-matrix, identity, u of its rows, v of its columns)."""
    c = clean(cost)
    perm = np.asarray(perm)
    keep = np.nonzero(c[np.arange(c.shape[0]), perm] < np.float32(FLT_MAX))[0]
    cols = perm[keep]
    return c[np.ix_(keep, cols)], np.arange(len(keep)), np.asarray(u)[keep], np.asarray(v)[cols]


def is_permutation(perm, n):
    return sorted(np.asarray(perm).tolist()) == list(range(n))


# ---- the cases ----------------------------------------------------------------------------------------------------------------
LDS_B = 192                                           # the kernel holds the matrix in LDS up to this batch (OT_LDS_B in csrc/ot.hip)
PAIR_CASES = [(1, 3), (7, 5), (64, 1024), (65, 37), (100, 4096), (LDS_B, 16), (LDS_B + 1, 16), (512, 64)]


def pair_case(B, D):
    """(source, target) fp32 [B, D]: a Gaussian source against a shifted, scaled Gaussian target."""
    g = np.random.default_rng(1000 * B + D)
    s = g.standard_normal((B, D)).astype(np.float32)
    t = (0.7 * g.standard_normal((B, D)) + 0.25).astype(np.float32)
    return s, t


def sqdist64(s, t):
    """|s_i - t_j|^2 in fp64."""
    s, t = s.astype(np.float64), t.astype(np.float64)
    out = np.empty((s.shape[0], t.shape[0]))
    for i in range(s.shape[0]):
        out[i] = ((s[i][None, :] - t) ** 2).sum(1)
    return out


def sqdist32(s, t):
    """The CPU stand-in for the device's matrix: fp32 differences, squares and sums (another summation order than the kernels')."""
    out = np.empty((s.shape[0], t.shape[0]), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(s.shape[0]):
            out[i] = ((s[i][None, :] - t) ** 2).sum(1, dtype=np.float32)
    return clean(out)


def tie_matrix(B, seed):
    """Integer-valued costs in 0..4: many ties."""
    return np.random.default_rng(seed).integers(0, 5, size=(B, B)).astype(np.float32)


def equal_matrix(B, value=3.0):
    return np.full((B, B), value, dtype=np.float32)


def greedy_trap(B=66):
    """[[1, 2], [2, 100]] in the corner of a matrix whose other rows have a free 0 on the diagonal and 1000 elsewhere: the row-by-row
    greedy sweep pays 1 + 100, the optimum 2 + 2."""
    c = np.full((B, B), 1000.0, dtype=np.float32)
    c[np.arange(B), np.arange(B)] = 0.0
    c[:2, :2] = [[1.0, 2.0], [2.0, 100.0]]
    return c, 4.0, 101.0


def random_matrix(B, seed):
    return np.random.default_rng(seed).random((B, B), dtype=np.float32)


TIE_CASES = [(7, 1), (40, 2), (66, 3), (130, 4), (200, 5)]          # (B, seed): every register count below 256 columns, both matrix homes


def hazard_case(kind="both"):
    """B = 70: a source row of NaN and a target row of inf ("both"), or only one of them ("row", "col").  With the column alone a finite
    row has to take a sentinel; with the row alone a finite column does."""
    g = np.random.default_rng(70)
    s = g.standard_normal((70, 32)).astype(np.float32)
    t = g.standard_normal((70, 32)).astype(np.float32)
    if kind in ("both", "row"):
        s[5] = np.nan
    if kind in ("both", "col"):
        t[40] = np.inf
    return s, t


def hazard_raw():
    """The hazard matrix with its sentinels put back as NaN / inf, and a lone -inf entry: what fc_ot_assign cleans by itself."""
    raw = sqdist32(*hazard_case()).copy()
    raw[5] = np.nan
    raw[:, 40] = np.inf
    raw[7, 3] = -np.inf
    return raw
