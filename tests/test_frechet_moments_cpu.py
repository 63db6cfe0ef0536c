"""The moment form's restatement (tests/frechet_moments_ref.py) against LAPACK on the concatenated rows, and the pieces of its bound
(DESIGN.md section 4 "Set distances -- the moment form").  tests/test_gpu_frechet_moments.py holds the device to the same functions."""
import numpy as np
import pytest

import frechet_moments_ref as MR
import frechet_ref as R


def sets_of(case):
    n1, n2, dim, kind = case
    if kind == "identical":
        x = np.array(R.gauss_sets(n1, n2, dim)[0])
        return x, x.copy()
    x, y = (np.array(v) for v in R.gauss_sets(n1, n2, dim))
    return MR.shifted((x, y)) if kind == "shifted" else (x, y)


def check(x, y, splits, label):
    a, b = MR.moments_of(x, splits[0]), MR.moments_of(y, splits[1])
    fd, info = MR.frechet_moments(a, b)
    want = R.frechet_lapack(x, y)
    parts = MR.moments_bound_parts(x, y, (a.batches, b.batches), info["evals"], info["svals"])
    print(f"\n[moments cpu] {label} {x.shape} {y.shape}: FD = {fd:.12e}, moment form - lapack = {fd - want:.3e} = "
          f"{abs(fd - want) / parts['total']:.2e} of the bound {parts['total']:.3e} (sample form's {R.frechet_bound(x, y):.3e}); sweeps {info['sweeps']}")
    assert info["converged"] and all(1 <= s <= R.MAX_SWEEPS for s in info["sweeps"])
    assert abs(fd - want) <= parts["total"]
    return fd, want, parts


FULL_RANK = ((300, 200, 36, "gauss"), (500, 400, 64, "gauss"), (64, 64, 48, "identical"), (300, 200, 36, "shifted"))


@pytest.mark.parametrize("case", FULL_RANK, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}-{c[3]}")
def test_full_rank_sets_in_uneven_batches_against_lapack(case):
    x, y = sets_of(case)
    fd, want, parts = check(x, y, (MR.uneven(len(x)), MR.uneven(len(y))), case[3])
    assert all(r < np.sqrt(np.sqrt(x.shape[1]) * e) for r, e in zip(parts["sqrt"], parts["eps"]))   # full rank: the Lipschitz branch, not the floor
    if case[3] == "identical":
        assert abs(fd) <= parts["total"] and want == pytest.approx(0.0, abs=parts["total"])


def test_fewer_samples_than_features_is_inside_the_bound_only_through_its_floor():
    """N < D: the covariances are singular, their zero eigenvalues come back as noise of size u ||S|| and the square roots of that noise
    enter the factors.  This is the moment form's documented weak side (the sample form's bound is orders of magnitude tighter here)."""
    x, y = sets_of((20, 30, 36, "gauss"))
    fd, want, parts = check(x, y, ((7, 1, 12), (30,)), "N < D")
    assert all(r == np.sqrt(np.sqrt(36) * e) for r, e in zip(parts["sqrt"], parts["eps"]))          # the floor branch on both sides
    assert parts["total"] > 100.0 * R.frechet_bound(x, y)


@pytest.mark.parametrize("splits", (None, MR.SPLITS, (1,) * 300), ids=("one-batch", "uneven", "single-rows"))
def test_the_same_set_in_different_batches(splits):
    x, y = sets_of((300, 200, 36, "gauss"))
    check(x, y, (splits, None), f"splits {splits if splits is None or len(splits) < 9 else '300 x 1'}")
    a = MR.moments_of(x, splits)
    n, dim, trs, amax = MR.set_scalars(x)
    err = float(np.linalg.norm(a.covariance() - MR.exact_covariance(x)))
    assert a.n == 300 and err <= MR.scatter_term(n, dim, a.batches, trs, amax)
    assert np.array_equal(a.M, a.M.T)


def test_chan_keeps_the_covariance_where_raw_moments_cancel():
    """A feature mean 100 sigma from zero: ss - n mu mu^T loses what Chan's centred scatters keep."""
    x = MR.shifted((np.array(R.gauss_sets(300, 200, 36)[0]),))[0]
    exact = MR.exact_covariance(x)
    n, dim, trs, amax = MR.set_scalars(x)
    chan = MR.moments_of(x, MR.SPLITS)
    e_chan, e_raw = (float(np.abs(c - exact).max()) for c in (chan.covariance(), MR.raw_covariance(x)))
    print(f"\n[moments cpu] mean at 100 sigma: max |S - exact| Chan {e_chan:.2e}, raw {e_raw:.2e}")
    assert float(np.linalg.norm(chan.covariance() - exact)) <= MR.scatter_term(n, dim, chan.batches, trs, amax)
    assert e_raw > 100.0 * e_chan


@pytest.mark.parametrize("n,dim", ((6, 2), (108, 36), (195, 65), (30, 36)))
def test_the_factor_reproduces_the_covariance(n, dim):
    x = np.array(R.gauss_sets(n, n, dim)[0])
    s = MR.moments_of(x).covariance()
    f, ev, sweeps, conv = MR.factor(s)
    fro = float(np.linalg.norm(s))
    lam = np.linalg.eigvalsh(s)[::-1]
    err, bound = float(np.linalg.norm(f.T @ f - s)), MR.factor_term(dim, fro, float(lam[0]), ev)
    print(f"\n[moments cpu] factor {n} x {dim}: ||F^T F - S||_F / ||S||_F = {err / fro:.2e}, {err / bound:.2e} of the term; sweeps {sweeps}")
    assert conv and err <= bound
    assert np.all(np.abs(ev - np.maximum(lam, 0.0)) <= R.svals_bound(dim, dim, fro, np.maximum(lam, 0.0), ev))


def test_merge_equals_sequential_updates():
    x, y = sets_of((300, 200, 36, "gauss"))
    seq = MR.moments_of(x, MR.SPLITS)
    left, right = MR.moments_of(x[:147], (17, 130)), MR.moments_of(x[147:], (1, 152))
    merged = MR.Moments().merge(left).merge(right)
    n, dim, trs, amax = MR.set_scalars(x)
    assert merged.n == seq.n == 300 and merged.batches == seq.batches == 4
    assert float(np.linalg.norm(merged.covariance() - seq.covariance())) <= 2.0 * MR.scatter_term(n, dim, 4, trs, amax)
    assert float(np.linalg.norm(merged.mean - seq.mean)) <= 2.0 * MR.mean_term(n, 4, amax)
    other = MR.moments_of(y)
    bound = MR.moments_bound(x, y, (4, 1))
    assert abs(MR.frechet_moments(merged, other)[0] - MR.frechet_moments(seq, other)[0]) <= 2.0 * bound
    assert abs(MR.frechet_moments(merged, other)[0] - R.frechet_lapack(x, y)) <= bound
