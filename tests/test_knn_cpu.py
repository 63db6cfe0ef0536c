"""What the nearest-neighbour work needs no GPU for: the fp64 restatement against scipy, PRDC against a case worked by hand, the host's
argument checks, and the properties of the shared inputs that tests/test_gpu_knn.py relies on."""
import numpy as np
import pytest
import torch

import knn_ref as R


def test_knn_ref_matches_scipy_on_tie_free_data():
    from scipy.spatial import cKDTree
    from scipy.spatial.distance import cdist
    rng = np.random.default_rng(0)
    for nq, n, dim, k in ((7, 50, 3, 5), (5, 40, 17, 40), (3, 9, 260, 1)):
        q, r = rng.standard_normal((nq, dim)), rng.standard_normal((n, dim))
        d2, idx = R.knn_ref(q, r, k)
        full = cdist(q, r, "sqeuclidean")
        order = np.argsort(full, axis=1)[:, :k]
        assert np.array_equal(idx, order)
        np.testing.assert_allclose(d2, np.take_along_axis(full, order, axis=1), rtol=1e-12)
        dist, tree_idx = cKDTree(r).query(q, k=k)
        assert np.array_equal(idx, np.asarray(tree_idx).reshape(nq, k))
        np.testing.assert_allclose(np.sqrt(d2), np.asarray(dist).reshape(nq, k), rtol=1e-12)
        rad = rng.uniform(0.5, 2.0, n) * dim
        assert np.array_equal(R.ball_counts_ref(q, r, rad), (full <= rad[None, :]).sum(axis=1))


def test_knn_ref_ties_exclusion_missing_slots_and_non_finite_rows():
    r = np.array([[1.0], [0.0], [1.0], [-1.0], [np.nan]])
    d2, idx = R.knn_ref(np.array([[0.0]]), r, 6, first_index=10)
    assert idx.tolist() == [[11, 10, 12, 13, 14, -1]]                     # ties by lower index, the NaN row last, one slot missing
    assert d2.tolist() == [[0.0, 1.0, 1.0, 1.0, R.FLT_MAX, np.inf]]
    d2, idx = R.knn_ref(np.array([[0.0]]), r, 2, query_ids=np.array([11]), first_index=10)
    assert idx.tolist() == [[10, 12]] and d2.tolist() == [[1.0, 1.0]]
    assert R.ball_counts_ref(np.array([[0.0]]), r, np.array([1.0, 0.0, 0.5, 1.0, np.inf]), query_ids=np.array([13]), first_index=10).tolist() == [3]


def test_prdc_ref_on_a_case_worked_by_hand():
    # real 0, 1, 6, 6.5 and fake 0.5, 2, 2.5 on a line, k = 1:
    #   r_real = 1, 1, .25, .25 (nearest other real, squared);  r_fake = 2.25, .25, .25
    #   d2(real_i, fake_j) = [[.25, 4, 6.25], [.25, 1, 2.25], [30.25, 16, 12.25], [36, 20.25, 16]]
    #   fake in real balls (<= r_real[i]):  (0,0), (1,0), (1,1)           -> precision 2/3, density 3 / (1 * 3)
    #   real in fake balls (<= r_fake[j]):  (0,0), (1,0)                  -> recall 2/4
    #   nearest fake within the real's own radius: real 0 and real 1     -> coverage 2/4
    real, fake = np.array([[0.0], [1.0], [6.0], [6.5]]), np.array([[0.5], [2.0], [2.5]])
    assert R.prdc_ref(real, fake, 1) == {"precision": 2 / 3, "recall": 0.5, "density": 1.0, "coverage": 0.5}
    same = R.prdc_ref(real, real, 1)                      # a set against itself: every ball holds its centre's copy and its nearest neighbour
    assert same == {"precision": 1.0, "recall": 1.0, "density": 2.0, "coverage": 1.0}


def test_host_argument_checks_and_cpu_tensors_raise():
    from flocoder_amd import metrics as M
    from flocoder_amd import neighbors as NB
    q, r = torch.zeros(3, 4), torch.zeros(5, 4)
    for bad_k in (0, 65, -1, 2.0, True):
        with pytest.raises(ValueError):
            NB.knn(q, r, bad_k)
        with pytest.raises(ValueError):
            NB.KnnSearch(q, bad_k)
    for call in (lambda: NB.knn(q, r, 1), lambda: NB.KnnSearch(q, 2), lambda: NB.ball_counts(q, r, torch.zeros(5)),
                 lambda: NB.nearest_in_dataset(q, [(r, None)]), lambda: M.prdc(q, r, 1)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    with pytest.raises(ValueError):
        NB.nearest_in_dataset(q, [(r, None)], chunk_rows=0)
    with pytest.raises(TypeError):
        NB.knn([[0.0]], r, 1)
    import inspect
    from flocoder_amd import sampling as S
    for fn in (M.compute_sample_metrics, S.evaluate_model):
        p = inspect.signature(fn).parameters["prdc_k"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None


def test_grid_inputs_are_exact_in_fp32_under_any_summation_order():
    for dim in R.DS:
        q, r = R.exact_case(65, 200, dim)
        both = np.concatenate([q, r])
        assert both.dtype == np.float32 and np.array_equal(both, np.round(both))
        worst = dim * (2.0 * np.abs(both).max()) ** 2                     # every partial sum is an integer no larger than this
        assert worst < 2 ** 24
        d2 = R.pairwise_d2(q, r)
        assert np.array_equal(d2, d2.astype(np.float32).astype(np.float64)) and np.array_equal(d2, np.round(d2))
    q, r = R.exact_case(2, 130, 4096)
    assert 4096 * (2.0 * np.abs(np.concatenate([q, r])).max()) ** 2 < 2 ** 24


def test_grid_inputs_tie_at_the_kth_place_for_at_least_half_the_queries():
    """Over all grid cases with more references than k, and in each 65-query case on its own where the grid is {-1, 0, 1} and N >= 63."""
    ties = total = 0
    for dim in R.DS:
        for n in R.NS:
            for nq in R.QS:
                q, r = R.exact_case(nq, n, dim)
                d2 = R.pairwise_d2(q, r)
                for k in R.KS:
                    if n <= k:
                        continue
                    d, _ = R.knn_ref(q, r, k + 1, d2=d2)
                    t = int((d[:, k - 1] == d[:, k]).sum())
                    ties, total = ties + t, total + nq
                    if dim <= 4 and n >= 63 and nq == 65:
                        assert 2 * t >= nq, (nq, n, dim, k, t)
    assert 2 * ties >= total, (ties, total)


def test_gaussian_ball_count_brackets_are_not_vacuous():
    """The GPU test lets a count lie anywhere between #{d (1 + e) <= r2} and #{d (1 - e) <= r2}: over its inputs the two differ in at most
    1 % of the counted pairs, pairs are counted at every dim and not every pair is."""
    upper = lower = pairs = 0
    for dim in R.DS:
        e = R.error_bound(dim)
        at_dim = 0
        for n in R.NS:
            for nq in R.QS:
                q, r = R.gauss_case(nq, n, dim)
                d2, rad = R.pairwise_d2(q, r), R.radii(r).astype(np.float64)
                lo, hi = int((d2 * (1 + e) <= rad).sum()), int((d2 * (1 - e) <= rad).sum())
                assert lo <= hi
                upper, lower, pairs, at_dim = upper + hi, lower + lo, pairs + d2.size, at_dim + lo
        assert at_dim > 0
    assert 0 < lower <= upper < pairs and (upper - lower) <= 0.01 * upper, (lower, upper, pairs)

