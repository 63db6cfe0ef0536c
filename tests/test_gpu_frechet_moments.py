"""flocoder_amd.distances.FrechetMoments / frechet_distance_moments and fid_score(solver="moments") on the device against the fp64
restatement, LAPACK and the sample form (tests/frechet_moments_ref.py, tests/frechet_ref.py).

Integer inputs with integer batch means come back bit for bit; Gaussian inputs within the bound derived in DESIGN.md section 4 "Set
distances -- the moment form" (frechet_moments_ref.scatter_term / factor_term / moments_bound).  tests/test_frechet_moments_cpu.py
checks what these tests rely on."""
import numpy as np
import pytest
import torch

import frechet_moments_ref as MR
import frechet_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NBS = (1, 2, 31, 32, 33, 65, 130)                  # both sides of the 32-row K chunk and of the MFMA's 4-row step
DIMS = (1, 3, 31, 32, 33, 65, 100)                 # both sides of the 32-wide tile and of the 16 x 16 block; 65 and 100: off-diagonal tiles


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)                     # a copy: the shared cases are read-only


def fed(x, splits=None):
    from flocoder_amd import distances as D
    st, r0, xd = D.FrechetMoments(), 0, dev(x)
    for nb in (splits or (len(x),)):
        st.update(xd[r0:r0 + nb])
        r0 += nb
    assert r0 == len(x) and st.n == len(x)
    return st


def integer_scatter(x):
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(axis=0)
    c = x - mean
    return mean, c.T @ c


# ---- scatter and merge, bit for bit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_scatter_of_integer_batches_is_bit_equal_to_numpy_and_symmetric(dim):
    for nb in NBS:
        x = R.dyadic_mean_case(nb, nb, dim)[0]
        mean, want = integer_scatter(x)
        assert np.array_equal(mean, np.round(mean)) and np.array_equal(want, np.round(want))     # the case is what it says
        st = fed(x)
        m = st.M.cpu()
        assert m.dtype == torch.float64 and m.shape == (dim, dim) and st.n == nb and st.dim == dim
        assert torch.equal(m, torch.from_numpy(want)), (nb, dim)
        assert torch.equal(m, m.t().contiguous()), (nb, dim)
        assert torch.equal(st.mean.cpu(), torch.from_numpy(mean)), (nb, dim)


def two_integer_batches(dim):
    """Two independently seeded 64-row batches with integer means; the second moved by an integer per column so that delta is not zero."""
    a = np.array(R.dyadic_mean_case(64, 64, dim, seed=0)[0])
    b = np.array(R.dyadic_mean_case(64, 64, dim, seed=1)[1]) + (np.arange(dim) % 3 * 2 - 1).astype(np.float32)
    return a, b


@pytest.mark.parametrize("dim", (33, 100))
def test_a_second_batch_and_a_merge_are_bit_equal_to_the_one_shot_integer_result(dim):
    from flocoder_amd import distances as D
    a, b = two_integer_batches(dim)
    assert np.any(a.mean(axis=0) != b.mean(axis=0))
    mean, want = integer_scatter(np.concatenate([a, b]))             # n = nb = 64: w = 32, the mean moves by delta / 2 -- all exact
    seq = fed(np.concatenate([a, b]), (64, 64))
    merged = D.FrechetMoments().merge(fed(a)).merge(fed(b))
    for st in (seq, merged):
        assert st.n == 128
        assert torch.equal(st.mean.cpu(), torch.from_numpy(mean))
        assert torch.equal(st.M.cpu(), torch.from_numpy(want)) and torch.equal(st.M, st.M.t().contiguous())
    assert merged.merge(D.FrechetMoments()).n == 128                 # an empty state adds nothing


def test_uneven_batches_against_the_one_shot_fp64_scatter():
    x = np.array(R.gauss_sets(300, 200, 100)[0])
    st = fed(x, MR.SPLITS)
    n, dim, trs, amax = MR.set_scalars(x)
    xc = x.astype(np.float64) - x.astype(np.float64).mean(axis=0)
    want = (xc.T @ xc) / (n - 1)
    got = st.covariance().cpu().numpy()
    err, bound = float(np.linalg.norm(got - want)), MR.scatter_term(n, dim, 4, trs, amax) + MR.scatter_term(n, dim, 1, trs, amax)
    print(f"\n[moments] uneven batches {MR.SPLITS} of {x.shape}: ||S - numpy||_F = {err:.3e} = {err / bound:.4f} of the scatter terms {bound:.3e}")
    assert err <= bound and np.array_equal(got, got.T)
    assert float(np.linalg.norm(st.mean.cpu().numpy() - x.astype(np.float64).mean(axis=0))) <= 2.0 * MR.mean_term(n, 4, amax)
    assert abs(st.trace() - float(np.trace(want))) <= np.sqrt(dim) * bound + dim * R.U * trs


# ---- factor ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (2, 36, 65, 130))
def test_factor_eigenvalues_and_product_against_the_covariance(dim):
    from flocoder_amd import distances as D
    n = 3 * dim
    x = np.array(R.gauss_sets(n, n, dim)[0])
    st = fed(x, (n - dim, dim))
    f, ev, info = st.factor()
    assert f.shape == (dim, dim) and ev.shape == (dim,) and f.dtype == ev.dtype == torch.float64
    assert info["converged"] and 1 <= info["sweeps"] <= R.MAX_SWEEPS and info["launches"] > 0
    got, s_dev = ev.cpu().numpy(), st.covariance().cpu().numpy()
    lam = np.linalg.eigvalsh(np.cov(x.astype(np.float64), rowvar=False).reshape(dim, dim))[::-1]
    _, _, trs, amax = MR.set_scalars(x)
    fro = float(np.linalg.norm(s_dev))
    per = MR.eigenvalue_bound(n, dim, 2, trs, amax, fro, lam, got)
    fn = f.cpu().numpy()
    err, term = float(np.linalg.norm(fn.T @ fn - s_dev)), MR.factor_term(dim, fro, float(lam[0]), got)
    print(f"\n[moments] factor D = {dim}: sweeps {info['sweeps']}, worst eigenvalue error {float(np.max(np.abs(got - lam) / per)):.4f} of its bound, "
          f"||F^T F - S||_F / ||S||_F = {err / fro:.2e} = {err / term:.4f} of the factor term")
    assert np.all(got[:-1] >= got[1:]) and np.all(np.abs(got - lam) <= per)
    assert err <= term
    assert abs(float(info["trace"]) - float(np.trace(s_dev))) <= dim * R.U * trs and st.trace() == float(info["trace"])
    # cached until the state changes; a state restored from the state dict factors to the same bits
    assert st.factor()[0] is f and st.factor()[1] is ev
    again = D.FrechetMoments().load_state_dict(st.state_dict())
    f2, ev2, _ = again.factor()
    assert f2 is not f and torch.equal(f2, f) and torch.equal(ev2, ev)
    st.update(dev(x[:5]))
    f3 = st.factor()[0]
    assert f3 is not f and st.n == n + 5 and not torch.equal(f3, f)


# ---- distance --------------------------------------------------------------------------------------------------------------------------
def check_distance(x, y, splits, label, sample_form=True):
    from flocoder_amd import distances as D
    a, b = fed(x, splits[0]), fed(y, splits[1])
    batches = tuple(len(s) if s else 1 for s in splits)
    fd, info = D.frechet_distance_moments(a, b, return_info=True)
    want = R.frechet_lapack(x, y)
    evals = (a.factor()[1].cpu().numpy(), b.factor()[1].cpu().numpy())
    bound = MR.moments_bound(x, y, batches, evals, info["svals"].cpu().numpy())
    cpu = MR.frechet_moments(MR.moments_of(x, splits[0]), MR.moments_of(y, splits[1]))[0]
    print(f"\n[moments] {label} {x.shape} {y.shape}: FD = {fd:.12e}, device - lapack = {fd - want:.3e} = {abs(fd - want) / bound:.2e} of the bound "
          f"{bound:.3e} (restatement - lapack = {cpu - want:.3e}); sweeps {info['sweeps']}, launches {info['launches']}")
    assert type(fd) is float and info["converged"] and len(info["sweeps"]) == 3 and all(1 <= s <= R.MAX_SWEEPS for s in info["sweeps"])
    assert abs(fd - want) <= bound
    assert D.frechet_distance_moments(a, b) == fd                                     # cached factors: the same bits
    assert D.frechet_distance_moments(fed(x, splits[0]), fed(y, splits[1])) == fd     # and from the rows again
    swapped, sinfo = D.frechet_distance_moments(b, a, return_info=True)
    assert abs(swapped - want) <= MR.moments_bound(y, x, batches[::-1], evals[::-1], sinfo["svals"].cpu().numpy())
    assert sinfo["trace_real"] == info["trace_fake"] and sinfo["trace_fake"] == info["trace_real"] and sinfo["mean_term"] == info["mean_term"]
    dm2, t1, t2, _ = R.frechet_parts(x, y)
    assert info["trace_real"] == a.trace() and info["trace_fake"] == b.trace()
    assert abs(info["trace_real"] - t1) + abs(info["trace_fake"] - t2) + abs(info["mean_term"] - dm2) <= bound
    assert abs((info["mean_term"] + info["trace_real"] + info["trace_fake"] - 2.0 * info["nuclear"]) - fd) <= 8 * R.U * (dm2 + t1 + t2)
    if sample_form:
        sets, sinfo = D.frechet_distance_sets(dev(x), dev(y), return_info=True)
        assert abs(fd - sets) <= bound + R.frechet_bound(x, y, sinfo["svals"].cpu().numpy())
    return fd, bound


@pytest.mark.parametrize("n1,n2,dim", ((300, 200, 36), (500, 400, 64), (400, 300, 130)))
def test_full_rank_gaussian_sets_against_lapack_and_the_sample_form(n1, n2, dim):
    x, y = (np.array(v) for v in R.gauss_sets(n1, n2, dim))
    check_distance(x, y, (MR.uneven(n1), None), "gauss")


def test_identical_sets_and_sets_far_from_the_origin():
    x = np.array(R.gauss_sets(64, 64, 48)[0])
    fd, bound = check_distance(x, x.copy(), (MR.uneven(64), None), "identical")
    assert abs(fd) <= bound < 1e-8                                   # the eigenvalue path: -2.8e-6
    x, y = MR.shifted(R.gauss_sets(300, 200, 36))
    check_distance(x, y, (MR.SPLITS, MR.uneven(200)), "every feature + 100")


def test_fewer_samples_than_features_only_inside_the_bound_with_its_floor_term():
    """The documented weak side of the moment form: for N < D the covariance is singular, its zero eigenvalues return as noise of size
    u ||S||, their square roots (size sqrt(u)) enter the factor, and only the floor branch of the bound holds.  The sample form
    (distances.frechet_distance_sets) is the right tool there, and DESIGN.md says so."""
    x, y = (np.array(v) for v in R.gauss_sets(20, 30, 36))
    parts = MR.moments_bound_parts(x, y)
    assert all(r == np.sqrt(6.0 * e) for r, e in zip(parts["sqrt"], parts["eps"]))
    check_distance(x, y, ((7, 1, 12), None), "N < D")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_non_finite_samples_and_limits_raise():
    from flocoder_amd import _binding as B
    from flocoder_amd import distances as D
    x, y = (np.array(v) for v in R.gauss_sets(300, 200, 36))
    good = fed(y)
    x[3, 7] = np.nan
    bad = fed(x, (100, 200))
    with pytest.raises(RuntimeError, match="did not converge"):
        bad.factor()
    with pytest.raises(RuntimeError, match="did not converge"):
        D.frechet_distance_moments(good, bad)
    ok = torch.zeros(4, 8, device=DEV)
    with pytest.raises(ValueError, match="4096"):
        D.FrechetMoments().update(torch.zeros(2, 4097, device=DEV))
    with pytest.raises(ValueError, match="features"):
        D.FrechetMoments().update(ok).update(torch.zeros(4, 9, device=DEV))
    with pytest.raises(ValueError, match="features"):
        D.frechet_distance_moments(good, D.FrechetMoments().update(ok))
    with pytest.raises(ValueError, match="features"):
        D.FrechetMoments().update(ok).merge(good)
    one = D.FrechetMoments().update(torch.zeros(1, 36, device=DEV))
    for call in (one.factor, one.covariance, one.trace, lambda: D.frechet_distance_moments(good, one), lambda: D.frechet_distance_moments(D.FrechetMoments(), good)):
        with pytest.raises(ValueError, match="at least 2"):
            call()
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.FrechetMoments().update(ok.cpu())
    with pytest.raises(TypeError):
        D.frechet_distance_moments(good, ok)
    # the library refuses the same before it launches anything: the outputs stay as they were
    lib, s = B.lib(), B.current_stream(ok.device)
    mean, m = torch.full((8,), -7.0, dtype=torch.float64, device=DEV), torch.full((8, 8), -7.0, dtype=torch.float64, device=DEV)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    sw, cv = B.C.c_int(-1), B.C.c_int(-1)
    for nb, dim, before in ((0, 8, 0), (65537, 8, 0), (4, 0, 0), (4, 4097, 0), (4, 8, -1)):
        assert lib.fc_frechet_moments_update(B.ptr(ok), nb, dim, before, B.ptr(mean), B.ptr(m), B.ptr(ws), s) == B.FC_E_SHAPE, (nb, dim, before)
    assert lib.fc_frechet_moments_update(None, 4, 8, 0, B.ptr(mean), B.ptr(m), B.ptr(ws), s) == B.FC_E_ARG
    assert lib.fc_frechet_moments_update(B.ptr(ok), 4, 8, 0, B.ptr(mean), B.ptr(m), ws.data_ptr() + 8, s) == B.FC_E_ARG
    assert lib.fc_frechet_moments_merge(8, 4, B.ptr(mean), B.ptr(m), 0, B.ptr(mean), B.ptr(m), B.ptr(ws), s) == B.FC_E_SHAPE
    assert lib.fc_frechet_moments_merge(4097, 4, B.ptr(mean), B.ptr(m), 4, B.ptr(mean), B.ptr(m), B.ptr(ws), s) == B.FC_E_SHAPE
    assert lib.fc_frechet_moments_factor(8, 1, B.ptr(m), B.ptr(m), B.ptr(mean), B.ptr(mean), B.ptr(ws), B.C.byref(sw), B.C.byref(cv), None, s) == B.FC_E_SHAPE
    assert lib.fc_frechet_moments_factor(8, 4, B.ptr(m), None, B.ptr(mean), B.ptr(mean), B.ptr(ws), B.C.byref(sw), B.C.byref(cv), None, s) == B.FC_E_ARG
    assert lib.fc_frechet_moments_distance(4097, B.ptr(mean), B.ptr(m), B.ptr(mean), B.ptr(mean), B.ptr(m), B.ptr(mean), B.ptr(ws), B.ptr(mean), None,
                                           B.C.byref(sw), B.C.byref(cv), None, s) == B.FC_E_SHAPE
    assert lib.fc_frechet_moments_distance(8, B.ptr(mean), B.ptr(m), B.ptr(mean), B.ptr(mean), None, B.ptr(mean), B.ptr(ws), B.ptr(mean), None,
                                           B.C.byref(sw), B.C.byref(cv), None, s) == B.FC_E_ARG
    for kind in (B.FC_WS_MOMENTS_UPDATE, B.FC_WS_MOMENTS_MERGE, B.FC_WS_MOMENTS_FACTOR, B.FC_WS_MOMENTS_DISTANCE):
        assert lib.fc_frechet_workspace_bytes(kind, 1, 1, 4097) == B.FC_E_SHAPE and lib.fc_frechet_workspace_bytes(kind, 1, 1, 4096) > 0
    assert lib.fc_frechet_workspace_bytes(B.FC_WS_MOMENTS_DISTANCE, 1, 1, 4096) > 4096 * 4096 * 8
    torch.cuda.synchronize()
    assert mean.tolist() == [-7.0] * 8 and m.flatten().tolist() == [-7.0] * 64 and sw.value == -1 and cv.value == -1


def test_state_dict_round_trip_and_rows_of_any_shape():
    from flocoder_amd import distances as D
    x, y = R.gauss_sets(300, 200, 36)
    a, b = fed(x), fed(y)
    sd = a.state_dict()
    assert set(sd) == {"n", "mean", "M"} and all(torch.is_tensor(v) for v in sd.values()) and int(sd["n"]) == 300
    back = D.FrechetMoments().load_state_dict({k: v.cpu() for k, v in sd.items()})    # as torch.load of a saved file gives them
    assert back.n == 300 and back.dim == 36 and torch.equal(back.M, a.M) and torch.equal(back.mean, a.mean)
    assert D.frechet_distance_moments(back, b) == D.frechet_distance_moments(a, b)
    shaped = D.FrechetMoments().update(dev(x).reshape(300, 4, 3, 3).double())          # any shape, any float type: flattened, cast to fp32
    assert torch.equal(shaped.M, a.M)


# ---- fid_score -------------------------------------------------------------------------------------------------------------------------
def test_fid_score_with_the_moments_solver():
    from flocoder_amd import distances as D
    from flocoder_amd import metrics as M

    def net(u8):                                                     # 16 x 16 -> 4 x 4 means of 16 bytes each: exact in fp32, 48 features
        return torch.nn.functional.avg_pool2d(u8.float(), 4)

    g = torch.Generator().manual_seed(5)
    real = torch.randn(150, 3, 16, 16, generator=g).to(DEV)
    fake = (torch.randn(120, 3, 16, 16, generator=g) * 1.2 + 0.1).to(DEV)
    got = M.fid_score(real, fake, device=DEV, inception=net, solver="moments")
    feats = [net(M.to_uint8(v)).reshape(len(v), -1) for v in (real, fake)]
    assert feats[0].shape == (150, 48)
    assert type(got) is float and got == D.frechet_distance_moments(D.FrechetMoments().update(feats[0]), D.FrechetMoments().update(feats[1]))
    fx, fy = (f.cpu().numpy() for f in feats)
    want, bound = R.frechet_lapack(fx, fy), MR.moments_bound(fx, fy, (5, 4))
    chunked = M.fid_score(real, fake, device=DEV, inception=net, solver="moments", chunk=True, chunk_size=37)
    print(f"\n[moments] fid_score: {got:.12e}, chunked {chunked:.12e}, lapack {want:.12e}, bound {bound:.3e}")
    assert abs(got - want) <= bound and abs(chunked - want) <= bound and abs(chunked - got) <= 2 * bound
    eig = M.fid_score(real, fake, device=DEV, inception=net)
    assert abs(got - eig) <= 1e-6 * abs(eig)
    with pytest.raises(ValueError):
        M.fid_score(real, fake, device=DEV, inception=net, solver="bogus")
