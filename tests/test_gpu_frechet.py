"""flocoder_amd.distances on the device against the fp64 restatement and LAPACK (tests/frechet_ref.py).

Exact inputs (small integers: every partial sum is exact in fp64 under any order) come back bit for bit; Gaussian inputs within the
bounds derived in DESIGN.md section 4 "Set distances" (frechet_ref.svals_bound / nuclear_bound / frechet_bound / kid_bound).
tests/test_frechet_cpu.py checks what these tests rely on."""
import numpy as np
import pytest
import torch

import frechet_ref as R
from conftest import load_golden
from oracle.synth import synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = (2, 15, 16, 17, 63, 65, 130)
DS = (1, 3, 4, 36, 260)


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)                     # a copy: the shared cases are read-only


# ---- Gram ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DS)
def test_gram_of_exact_inputs_is_bit_equal_to_numpy(dim):
    from flocoder_amd import distances as D
    for n1 in NS:
        for n2 in NS:
            a, b = R.exact_case(n1, n2, dim)                         # b is not a's transpose or a symmetric partner: a swapped row / column map shows
            got = D.gram(dev(a), dev(b))
            assert got.dtype == torch.float64 and got.shape == (n1, n2)
            assert torch.equal(got.cpu(), torch.from_numpy(R.gram64(a, b))), (n1, n2, dim)
            a, b = R.dyadic_mean_case(n1, n2, dim)
            got = D.gram(dev(a), dev(b), center=True)
            assert torch.equal(got.cpu(), torch.from_numpy(R.gram64(a, b, center=True))), (n1, n2, dim, "centred")


# ---- Jacobi --------------------------------------------------------------------------------------------------------------------------
def test_diagonal_and_orthogonal_inputs_return_the_exact_norms_in_one_sweep():
    from flocoder_amd import distances as D
    diag = np.diag([3.0, 0.5, 7.0, 2.0, 0.25, 11.0])
    sv, info = D.singular_values(dev(diag))
    assert info["converged"] and info["sweeps"] == 1 and sv.tolist() == [11.0, 7.0, 3.0, 2.0, 0.5, 0.25] and float(info["nuclear"]) == 23.75
    had = np.array([[1, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1]], dtype=np.float64) * np.array([[3.0], [1.0], [2.0], [0.5]])
    sv, info = D.singular_values(dev(had))                           # orthogonal rows of norms 6, 2, 4, 1
    assert info["converged"] and info["sweeps"] == 1 and sv.tolist() == [6.0, 4.0, 2.0, 1.0]


def test_the_zero_matrix_returns_zeros():
    from flocoder_amd import distances as D
    sv, info = D.singular_values(torch.zeros(7, 5, dtype=torch.float64, device=DEV))
    assert info["converged"] and info["sweeps"] == 1 and sv.tolist() == [0.0] * 7 and float(info["nuclear"]) == 0.0


def check_against_lapack(m, label):
    from flocoder_amd import distances as D
    n, r = m.shape
    want = np.zeros(n)
    lap = np.linalg.svd(m, compute_uv=False)
    want[:len(lap)] = lap
    md = dev(m)
    sv, info = D.singular_values(md)
    assert torch.equal(md.cpu(), torch.from_numpy(np.ascontiguousarray(m)))          # the caller's matrix is not the one destroyed
    got, fro = sv.cpu().numpy(), float(np.linalg.norm(m))
    assert info["converged"] and 1 <= info["sweeps"] <= R.MAX_SWEEPS and got.shape == (n,) and np.all(got[:-1] >= got[1:])
    per, tot = R.svals_bound(n, r, fro, want, got), R.nuclear_bound(n, r, fro, float(want.sum()), got)
    e_per, e_tot = np.abs(got - want), abs(float(info["nuclear"]) - float(want.sum()))
    print(f"\n[jacobi] {label} {n} x {r}: sweeps {info['sweeps']}, worst per-value error {float(np.max(e_per / per)):.4f} of its bound, "
          f"sum error {e_tot:.3e} = {e_tot / tot:.4f} of the bound {tot:.3e}")
    assert np.all(e_per <= per) and e_tot <= tot
    assert abs(float(info["nuclear"]) - float(got.sum())) <= n * R.U * want.sum()   # the sum returned is the sum of the values returned
    return info


@pytest.mark.parametrize("n,r,rank", R.JACOBI_CASES + ((5, 3, None), (63, 65, None)))
def test_gaussian_matrices_against_lapack(n, r, rank):
    """(5, 3) and (63, 65): odd n, where the padding vector sits out one pair per round."""
    check_against_lapack(np.array(R.gauss_matrix(n, r, rank)), f"rank {rank}")


def test_rank_far_below_the_number_of_vectors():
    check_against_lapack(np.array(R.gauss_matrix(64, 3)), "r = 3")


def test_vectors_longer_than_the_lds_resident_form_take_the_two_pass_path():
    from flocoder_amd import distances as D
    r = D.LDS_R + 1                                                  # FC_JACOBI_LDS_R + 1: the smallest r whose pair does not fit the carve
    check_against_lapack(np.array(R.gauss_matrix(4, r)), "two-pass")
    check_against_lapack(np.array(R.gauss_matrix(4, D.LDS_R)), "largest LDS-resident")


def test_a_nan_entry_ends_without_convergence_and_the_distance_raises():
    from flocoder_amd import distances as D
    m = np.array(R.gauss_matrix(48, 64, 31))
    m[17, 5] = np.nan
    _, info = D.singular_values(dev(m))
    assert info["converged"] is False and info["sweeps"] == 1
    x, y = (np.array(v) for v in R.gauss_sets(63, 65, 36))
    y[3, 7] = np.nan
    with pytest.raises(RuntimeError, match="did not converge"):
        D.frechet_distance_sets(dev(x), dev(y))
    x[1, 1] = np.inf
    with pytest.raises(RuntimeError, match="did not converge"):
        D.frechet_distance_sets(dev(x), dev(x))


# ---- Frechet -------------------------------------------------------------------------------------------------------------------------
def check_frechet(x, y, label):
    from flocoder_amd import distances as D
    xd, yd = dev(x), dev(y)
    fd, info = D.frechet_distance_sets(xd, yd, return_info=True)
    want = R.frechet_lapack(x, y)
    bound = R.frechet_bound(x, y, info["svals"].cpu().numpy())
    print(f"\n[frechet] {label} {x.shape} {y.shape}: FD = {fd:.12e}, lapack {want:.12e}, |diff| = {abs(fd - want):.3e} = "
          f"{abs(fd - want) / bound:.4f} of the bound {bound:.3e}; sweeps {info['sweeps']}, launches {info['launches']}")
    assert type(fd) is float and info["converged"] and 1 <= info["sweeps"] <= R.MAX_SWEEPS
    assert abs(fd - want) <= bound
    assert D.frechet_distance_sets(xd, yd) == fd                      # twice in a row: the same bits
    swapped = D.frechet_distance_sets(yd, xd)
    assert abs(swapped - fd) <= 2 * bound
    dm2, t1, t2, _ = R.frechet_parts(x, y)
    tol = (max(len(x), len(y)) + x.shape[1] + 8) * R.U
    assert abs(info["mean_term"] - dm2) <= tol * max(dm2, t1 + t2) and abs(info["trace_real"] - t1) <= tol * t1 and abs(info["trace_fake"] - t2) <= tol * t2
    return fd, bound


@pytest.mark.parametrize("n1,n2,dim", R.FRECHET_SHAPES)
def test_frechet_distance_against_the_lapack_form(n1, n2, dim):
    x, y = R.gauss_sets(n1, n2, dim)
    check_frechet(x, y, "gauss")


def test_frechet_distance_of_near_identical_and_identical_sets():
    x, y = R.near_identical_sets(64, 128, 1e-3)
    fd, bound = check_frechet(x, y, "noise 1e-3")
    assert fd > 100 * bound                                          # 9.9e-5: resolved, where the eigenvalue path is 3 % off
    fd, bound = check_frechet(x, x, "identical")
    assert abs(fd) <= bound < 1e-8                                   # the eigenvalue path: -2.8e-6


def test_samples_of_any_shape_are_flattened():
    from flocoder_amd import distances as D
    x, y = R.gauss_sets(17, 15, 36)
    assert D.frechet_distance_sets(dev(x).reshape(17, 4, 3, 3), dev(y).reshape(15, 4, 3, 3)) == D.frechet_distance_sets(dev(x), dev(y))
    assert D.kernel_distance(dev(x).reshape(17, 4, 3, 3), dev(y).reshape(15, 4, 3, 3)) == D.kernel_distance(dev(x), dev(y))


# ---- KID -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2,dim", R.FRECHET_SHAPES)
def test_kernel_distance_against_the_restatement(n1, n2, dim):
    from flocoder_amd import distances as D
    x, y = R.gauss_sets(n1, n2, dim)
    xd, yd = dev(x), dev(y)
    got, want, bound = D.kernel_distance(xd, yd), R.kid_ref(x, y), R.kid_bound(x, y)
    print(f"\n[kid] {x.shape} {y.shape}: {got:.12e}, fp64 {want:.12e}, |diff| = {abs(got - want):.3e} = {abs(got - want) / bound:.4f} of the bound {bound:.3e}")
    assert type(got) is float and abs(got - want) <= bound
    assert D.kernel_distance(xd, yd) == got
    xi, yi = R.exact_case(n1, n2, dim)                               # exact sums of k need integers small enough: g / D is not an integer, so
    gi = D.kernel_distance(dev(xi), dev(yi))                         # this one is held to the bound as well
    assert abs(gi - R.kid_ref(xi, yi)) <= R.kid_bound(xi, yi)


def test_kernel_distance_of_a_set_against_its_permutation():
    from flocoder_amd import distances as D
    x, _ = R.gauss_sets(65, 63, 36)
    xp = x[np.random.default_rng(3).permutation(65)]
    k = ((x.astype(np.float64) @ x.astype(np.float64).T) / 36 + 1.0) ** 3
    want = 2.0 / 65 * ((k.sum() - np.trace(k)) / (65 * 64.0) - np.trace(k) / 65)      # tests/test_frechet_cpu.py has the closed form
    assert abs(D.kernel_distance(dev(x), dev(xp)) - want) <= R.kid_bound(x, xp)


# ---- limits --------------------------------------------------------------------------------------------------------------------------
def test_limits_raise_the_documented_errors_without_a_launch():
    from flocoder_amd import _binding as B
    from flocoder_amd import distances as D
    lib = B.lib()
    ok = torch.zeros(4, 8, device=DEV)
    with pytest.raises(ValueError, match="4096"):
        D.frechet_distance_sets(torch.zeros(4097, 2, device=DEV), torch.zeros(4097, 2, device=DEV))
    for fn in (D.frechet_distance_sets, D.kernel_distance):
        with pytest.raises(ValueError, match="at least 2"):
            fn(torch.zeros(1, 8, device=DEV), ok)
        with pytest.raises(ValueError, match="features"):
            fn(ok, torch.zeros(4, 9, device=DEV))
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(ok.cpu(), ok)
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.gram(ok, ok.cpu())
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.singular_values(torch.zeros(3, 3, dtype=torch.float64))
    with pytest.raises(ValueError):
        D.singular_values(torch.zeros(3, 3, device=DEV))             # fp32
    with pytest.raises(ValueError):
        D.singular_values(torch.zeros(4097, 2, dtype=torch.float64, device=DEV))
    # the library refuses the same before it launches anything: the outputs stay as they were
    out, ws = torch.full((6,), -7.0, dtype=torch.float64, device=DEV), torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    sw, cv = B.C.c_int(-1), B.C.c_int(-1)
    s = B.current_stream(ok.device)
    for n1, n2, dim in ((1, 4, 8), (4, 1, 8), (4, 4, 0), (4097, 4097, 8), (4, 16385, 8)):
        rc = lib.fc_frechet_sets(B.ptr(ok), n1, B.ptr(ok), n2, dim, B.ptr(ws), B.ptr(out), None, B.C.byref(sw), B.C.byref(cv), None, s)
        assert rc == B.FC_E_SHAPE, (n1, n2, dim)
        with pytest.raises(ValueError):
            B.check(rc)
    assert lib.fc_kid_sets(B.ptr(ok), 4, B.ptr(ok), 16385, 8, B.ptr(ws), B.ptr(out), s) == B.FC_E_SHAPE
    assert lib.fc_kid_sets(B.ptr(ok), 1, B.ptr(ok), 4, 8, B.ptr(ws), B.ptr(out), s) == B.FC_E_SHAPE
    assert lib.fc_frechet_sets(None, 4, B.ptr(ok), 4, 8, B.ptr(ws), B.ptr(out), None, B.C.byref(sw), B.C.byref(cv), None, s) == B.FC_E_ARG
    assert lib.fc_frechet_sets(B.ptr(ok), 4, B.ptr(ok), 4, 8, None, B.ptr(out), None, B.C.byref(sw), B.C.byref(cv), None, s) == B.FC_E_ARG
    assert lib.fc_jacobi_svals(B.ptr(out), 4097, 1, B.ptr(out), None, B.ptr(ws), B.C.byref(sw), B.C.byref(cv), s) == B.FC_E_SHAPE
    assert lib.fc_gram_f64(B.ptr(ok), 0, B.ptr(ok), 4, 8, None, None, 1.0, B.ptr(out), None, None, s) == B.FC_E_SHAPE
    assert lib.fc_frechet_workspace_bytes(B.FC_WS_FRECHET, 4097, 4097, 8) == B.FC_E_SHAPE
    assert lib.fc_frechet_workspace_bytes(B.FC_WS_FRECHET, 4096, 16384, 8) > 4096 * 16384 * 8
    torch.cuda.synchronize()
    assert out.tolist() == [-7.0] * 6 and sw.value == -1 and cv.value == -1


# ---- wiring --------------------------------------------------------------------------------------------------------------------------
def small_models():
    """The models of tests/test_gpu_eval_metrics.py."""
    from flocoder_amd.codecs import VQVAE
    from flocoder_amd.unet import Unet
    torch.manual_seed(0)
    model = Unet(dim=8, dim_mults=(1, 2, 4, 8), channels=4, n_classes=10).to(DEV)
    codec = VQVAE(vq_num_embeddings=64, codebook_levels=3, in_channels=1, hidden_channels=32, num_downsamples=4, internal_dim=32,
                  vq_embedding_dim=4).eval()
    codec.load_state_dict(synth_state_dict(load_golden("g9_vqvae")["gray_nd4_small_shapes"], 9), strict=False)
    gen = torch.Generator().manual_seed(1)
    for i in range(3):
        codec.vq.layers[i]._codebook.embed.copy_(torch.randn(1, 64, 4, generator=gen) * (0.5 ** i))
        codec.vq.layers[i]._codebook.initted.fill_(True)
    return model, codec.to(DEV)


PLAIN_KEYS = {"sinkhorn", "sinkhorn_px", "mse", "mse_px", "pred_mean", "targ_mean", "pred_std", "targ_std", "pred_px_mean", "targ_px_mean",
              "pred_px_std", "targ_px_std"}
NEW_KEYS = {"frechet", "frechet_px", "kid", "kid_px"}


def test_evaluate_model_and_compute_sample_metrics_add_four_keys_and_change_nothing_else():
    from flocoder_amd import distances as D
    from flocoder_amd import metrics as M
    from flocoder_amd import sampling as S
    model, codec = small_models()
    g = torch.Generator().manual_seed(7)
    bsz, steps = 7, 2
    target = torch.randn(9, 4, 8, 8, generator=g).to(DEV)
    source = torch.randn(bsz, 4, 8, 8, generator=g).to(DEV)
    kw = dict(batch_size=bsz, method="rk4", n_steps=steps, is_midi=True, source=source)
    plain = S.evaluate_model(model, codec, 0, target, **kw)
    assert set(plain) == PLAIN_KEYS | {k for k in plain if k.startswith("note/")}
    got, images = S.evaluate_model(model, codec, 0, target, frechet=True, kid=True, return_images=True, **kw)
    assert set(got) == set(plain) | NEW_KEYS
    for k, v in plain.items():
        assert type(got[k]) is float and got[k] == v, (k, got[k], v)
    pred, dp, dt = images["pred_latents"], images["decoded_pred"], images["decoded_target"]
    want = {"frechet": D.frechet_distance_sets(target[:bsz], pred), "frechet_px": D.frechet_distance_sets(dt, dp),
            "kid": D.kernel_distance(target[:bsz], pred), "kid_px": D.kernel_distance(dt, dp)}
    for k, v in want.items():
        assert type(got[k]) is float and got[k] == v, (k, got[k], v)
    only_kid = S.evaluate_model(model, codec, 0, target, kid=True, **kw)
    assert set(only_kid) == set(plain) | {"kid", "kid_px"}
    # compute_sample_metrics itself (it rescales decoded_pred in place: every call gets its own copy)
    base = M.compute_sample_metrics(pred, target, dp.clone(), dt)
    both = M.compute_sample_metrics(pred, target, dp.clone(), dt, frechet=True, kid=True)
    assert set(base) == PLAIN_KEYS and set(both) == PLAIN_KEYS | NEW_KEYS
    assert all(both[k] == base[k] for k in base) and all(type(both[k]) is float for k in NEW_KEYS)


def test_fid_score_with_the_jacobi_solver_agrees_with_the_eigenvalue_form_on_full_rank_features():
    from flocoder_amd import metrics as M
    g = torch.Generator().manual_seed(5)
    proj = (torch.randn(3 * 8 * 8, 16, generator=g) / 255.0).to(DEV)                  # a fixed random projection as the feature network

    def net(u8):
        return u8.reshape(u8.shape[0], -1).float() @ proj

    real = torch.randn(200, 3, 8, 8, generator=g).to(DEV)
    fake = (torch.randn(180, 3, 8, 8, generator=g) * 1.2 + 0.1).to(DEV)
    eig = M.fid_score(real, fake, device=DEV, inception=net)
    jac = M.fid_score(real, fake, device=DEV, inception=net, solver="jacobi")
    assert type(jac) is float and abs(jac - eig) <= 1e-6 * abs(eig), (jac, eig)
    chunked = M.fid_score(real, fake, device=DEV, inception=net, solver="jacobi", chunk=True, chunk_size=64)     # the features' own fp32 rounding may move
    assert abs(chunked - jac) <= 1e-6 * abs(eig)
    with pytest.raises(ValueError):
        M.fid_score(real, fake, device=DEV, inception=net, solver="qr")
