"""The restatement tests/frechet_ref.py against LAPACK, against the existing metrics.frechet_distance where that one can be trusted,
and against closed forms -- what tests/test_gpu_frechet.py relies on.  No GPU.

Measured (fp64, CPU): the restated Jacobi against np.linalg.svd on ||M||_* is at most 1.8e-14 relative over JACOBI_CASES (1.3e-10
absolute at 128 x 128 rank 63), at most 0.0026 of nuclear_bound; sweeps 2 .. 12."""
import math

import numpy as np
import pytest
import torch

import frechet_ref as R


@pytest.mark.parametrize("n,r,rank", R.JACOBI_CASES)
def test_restated_jacobi_agrees_with_lapack_within_the_derived_bound(n, r, rank):
    m = R.gauss_matrix(n, r, rank)
    want = np.linalg.svd(m, compute_uv=False)
    got, sweeps, conv = R.jacobi_svals(m)
    fro = float(np.linalg.norm(m))
    assert conv and sweeps <= R.MAX_SWEEPS and got.shape == (n,)
    bound = R.nuclear_bound(n, r, fro, float(want.sum()), got)
    err = abs(float(got.sum()) - float(want.sum()))
    print(f"\n[jacobi ref] {n} x {r} rank {rank}: sweeps {sweeps}, |nuclear - lapack| = {err:.3e} = {err / want.sum():.2e} relative, "
          f"{err / bound:.4f} of the bound {bound:.3e}")
    assert err <= bound
    full = np.zeros(n)
    full[:len(want)] = want
    assert np.all(np.abs(got - full) <= R.svals_bound(n, r, fro, full, got))
    assert bound <= 1e-9 * want.sum()                               # the bound itself says something: nine digits of the nuclear norm


def test_schedule_meets_every_pair_once_per_sweep():
    for m in (2, 4, 6, 48, 130):
        seen = set()
        for rnd in range(m - 1):
            ia, ib = R.round_pairs(m, rnd)
            assert len(set(ia.tolist()) | set(ib.tolist())) == m    # a round's pairs are disjoint
            seen |= set(zip(ia.tolist(), ib.tolist()))
        assert seen == {(i, j) for i in range(m) for j in range(i + 1, m)}


def test_the_floor_spares_sweeps_on_a_rank_deficient_matrix():
    m = R.gauss_matrix(128, 128, 63)
    with_floor, without = R.jacobi_svals(m), R.jacobi_svals(m, floor=False)
    assert with_floor[2] and with_floor[1] <= without[1]
    assert abs(with_floor[0].sum() - without[0].sum()) <= R.nuclear_bound(128, 128, float(np.linalg.norm(m)), float(with_floor[0].sum()), with_floor[0])


def test_identity_against_the_existing_frechet_distance_on_full_rank_inputs():
    """N = 400 > D = 32: both covariances have full rank, the one regime where eigvals(S1 S2) can be trusted."""
    from flocoder_amd import metrics as M
    x, y = R.gauss_sets(400, 400, 32)
    stats = (M.FrechetStatistics(), M.FrechetStatistics())
    stats[0].update(torch.from_numpy(x.copy()))
    stats[1].update(torch.from_numpy(y.copy()))
    old = M.frechet_distance(*stats[0].moments(), *stats[1].moments())
    for new in (R.frechet_lapack(x, y), R.frechet_jacobi(x, y)[0]):
        assert abs(new - old) <= 1e-9 * abs(old), (new, old)


def test_identical_sets_give_zero_within_the_bound():
    """64 x 128, the case on which the existing path (FrechetStatistics + frechet_distance, fp64, CPU) returns -2.8e-6: both covariances
    are singular and eigvals(S1 S2).sqrt().real drops what came out negative or complex.  Here: |FD| <= the bound, about 1e-10."""
    x, _ = R.near_identical_sets(64, 128, 0.0)
    fd, sweeps, conv = R.frechet_jacobi(x, x)
    bound = R.frechet_bound(x, x)
    print(f"\n[frechet ref] identical 64 x 128: FD = {fd:.3e}, bound {bound:.3e}, sweeps {sweeps}")
    assert conv and abs(fd) <= bound and bound < 1e-8
    assert abs(R.frechet_lapack(x, x)) <= bound


def test_near_identical_sets_agree_with_lapack():
    x, y = R.near_identical_sets(64, 128, 1e-3)
    fd, _, conv = R.frechet_jacobi(x, y)
    want = R.frechet_lapack(x, y)
    assert conv and abs(fd - want) <= R.frechet_bound(x, y)
    assert 5e-5 < want < 2e-4                                       # 9.9e-5 in the issue's experiment: a distance far above the bound


@pytest.mark.parametrize("n1,n2,dim", R.FRECHET_SHAPES)
def test_frechet_restatement_on_the_gpu_tests_shapes(n1, n2, dim):
    x, y = R.gauss_sets(n1, n2, dim)
    fd, sweeps, conv = R.frechet_jacobi(x, y)
    assert conv and abs(fd - R.frechet_lapack(x, y)) <= R.frechet_bound(x, y)
    swapped = R.frechet_jacobi(y, x)[0]
    assert abs(fd - swapped) <= 2 * R.frechet_bound(x, y)


def test_kid_of_a_set_against_its_own_permutation_is_the_estimators_known_value():
    """X against a permutation of X: with S_off = sum_{i != j} k_ij and S_diag = sum_i k_ii,
    MMD^2 = 2 S_off / (N (N - 1)) - 2 (S_off + S_diag) / N^2 = (2 / N) (mean off-diagonal k - mean diagonal k): negative, not zero."""
    x, _ = R.gauss_sets(65, 63, 36)
    n, d = x.shape
    xp = x[np.random.default_rng(3).permutation(n)]
    k = ((x.astype(np.float64) @ x.astype(np.float64).T) / d + 1.0) ** 3
    off, diag = (k.sum() - np.trace(k)) / (n * (n - 1.0)), np.trace(k) / n
    want = 2.0 / n * (off - diag)
    got = R.kid_ref(x, xp)
    assert want < 0 and abs(got - want) <= R.kid_bound(x, xp)


def test_exact_cases_are_exact():
    for gen in (R.exact_case, R.dyadic_mean_case):
        a, b = gen(130, 63, 260)
        assert np.abs(a).max() <= 3 * 130 + 2 and np.all(a == np.round(a)) and np.all(b == np.round(b))
    a, b = R.dyadic_mean_case(130, 63, 260)
    assert np.all(a.astype(np.float64).mean(axis=0) == (np.arange(260) % 5 - 2)) and np.all(b.astype(np.float64).sum(axis=0) == 63 * (np.arange(260) % 5 - 2))
    g = R.gram64(a, b, center=True)
    assert np.all(g == np.round(g)) and np.abs(g).max() < 2.0 ** 40
    assert not math.isnan(R.kid_ref(a, b))
