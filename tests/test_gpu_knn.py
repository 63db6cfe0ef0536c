"""flocoder_amd.neighbors and metrics.prdc on the device against the fp64 restatement (tests/knn_ref.py).

Exact inputs (small integers: every partial sum exact in fp32 under any order) must come back bit for bit; Gaussian inputs within the
derived bound e(D) = (D + 2) 2^-24 / (1 - (D + 2) 2^-24), which holds for any summation order because every term is non-negative.
tests/test_knn_cpu.py checks what these tests rely on: exactness and ties of the grid inputs, and that the ball-count bracket is tight."""
import numpy as np
import pytest
import torch

import knn_ref as R
from conftest import load_golden
from oracle.synth import synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLT_MAX = torch.finfo(torch.float32).max


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def exclusions(nq, n, first):
    """One global index per query, inside the chunk for most queries and outside it for some."""
    return (np.arange(nq, dtype=np.int64) * 7) % (n + 2) + first


@pytest.mark.parametrize("dim", R.DS)
def test_exact_inputs_come_back_bit_for_bit(dim):
    from flocoder_amd import neighbors as NB
    for n in R.NS:
        for nq in R.QS:
            q, r = R.exact_case(nq, n, dim)
            qd, rd, d2 = dev(q), dev(r), R.pairwise_d2(q, r)
            ids = exclusions(nq, n, 3)
            for k in R.KS:
                got_d, got_i = NB.knn(qd, rd, k)
                want_d, want_i = R.knn_ref(q, r, k, d2=d2)
                assert got_d.dtype == torch.float32 and got_i.dtype == torch.int64 and got_d.shape == got_i.shape == (nq, k)
                assert torch.equal(got_i.cpu(), torch.from_numpy(want_i)), (nq, n, dim, k)      # ties by lower index, -1 in missing slots
                assert torch.equal(got_d.cpu(), torch.from_numpy(want_d.astype(np.float32))), (nq, n, dim, k)
                got_d, got_i = NB.KnnSearch(qd, k, query_ids=dev(ids)).update(rd, first_index=3).result()
                want_d, want_i = R.knn_ref(q, r, k, query_ids=ids, first_index=3, d2=d2)
                assert torch.equal(got_i.cpu(), torch.from_numpy(want_i)), (nq, n, dim, k, "query_ids")
                assert torch.equal(got_d.cpu(), torch.from_numpy(want_d.astype(np.float32))), (nq, n, dim, k, "query_ids")
            rad = R.radii(r)
            got = NB.ball_counts(qd, rd, dev(rad))
            assert got.dtype == torch.int32 and got.cpu().tolist() == R.ball_counts_ref(q, r, rad, d2=d2).tolist(), (nq, n, dim)
            got = NB.ball_counts(qd, rd, dev(rad), query_ids=dev(ids), first_index=3)
            assert got.cpu().tolist() == R.ball_counts_ref(q, r, rad, query_ids=ids, first_index=3, d2=d2).tolist(), (nq, n, dim, "query_ids")


@pytest.mark.parametrize("dim,n,m,k", [(4, 65, 63, 5), (36, 200, 65, 5), (3, 4, 3, 5), (260, 63, 65, 1)])
def test_prdc_equals_restatement_on_exact_inputs(dim, n, m, k):
    from flocoder_amd import metrics as M
    real, fake = R.exact_case(n, m, dim)
    got = M.prdc(dev(real), dev(fake), k)
    assert all(type(v) is float for v in got.values())
    assert got == R.prdc_ref(real, fake, k)


@pytest.mark.parametrize("dim", R.DS)
def test_gaussian_inputs_within_the_derived_bound(dim):
    from flocoder_amd import neighbors as NB
    e, worst = R.error_bound(dim), 0.0
    for n in R.NS:
        for nq in R.QS:
            q, r = R.gauss_case(nq, n, dim)
            qd, rd, d2 = dev(q), dev(r), R.pairwise_d2(q, r)
            for k in R.KS:
                got_d, got_i = (t.cpu().numpy() for t in NB.knn(qd, rd, k))
                m = min(k, n)
                assert np.all(got_i[:, m:] == -1) and np.all(np.isposinf(got_d[:, m:]))
                for row in range(nq):                                                  # no query is left out of any check
                    idx, dt = got_i[row, :m], got_d[row, :m].astype(np.float64)
                    assert idx.min() >= 0 and idx.max() < n and len(set(idx.tolist())) == m
                    exact = d2[row, idx]
                    assert np.all(np.abs(dt - exact) <= e * exact), (nq, n, dim, k, row)
                    worst = max(worst, float(np.max(np.abs(dt - exact) / (e * exact))))
                    assert np.all((dt[1:] > dt[:-1]) | ((dt[1:] == dt[:-1]) & (idx[1:] > idx[:-1]))), (nq, n, dim, k, row)
                    rest = np.ones(n, dtype=bool)
                    rest[idx] = False
                    assert np.all(d2[row, rest] * (1 + e) >= dt[-1]), (nq, n, dim, k, row)
            rad = R.radii(r)
            got = NB.ball_counts(qd, rd, dev(rad)).cpu().numpy()
            lo, hi = (d2 * (1 + e) <= rad.astype(np.float64)).sum(axis=1), (d2 * (1 - e) <= rad.astype(np.float64)).sum(axis=1)
            assert np.all((lo <= got) & (got <= hi)), (nq, n, dim)
    print(f"\n[knn] dim {dim}: largest |d2 - exact| = {worst:.4f} of the bound e = {e:.3e}")


@pytest.mark.parametrize("dim,exact", [(4, True), (36, False), (260, False)])
def test_chunked_updates_in_any_order_give_the_bits_of_one_call(dim, exact):
    from flocoder_amd import neighbors as NB
    q, r = (R.exact_case if exact else R.gauss_case)(65, 200, dim)
    qd, rd = dev(q), dev(r)
    ids = dev(exclusions(65, 200, 0))
    for k in (5, 64):
        for query_ids in (None, ids):
            one_d, one_i = NB.knn(qd, rd, k, query_ids=query_ids)
            for step in (63, 4 if k == 5 else 50):                 # 63 and 50: k = 64 across chunks smaller than k
                search = NB.KnnSearch(qd, k, query_ids=query_ids)
                for lo in reversed(range(0, 200, step)):           # fed in reverse order
                    search.update(rd[lo:lo + step], first_index=lo)
                d, i = search.result()
                assert torch.equal(i, one_i) and torch.equal(d, one_d), (dim, k, step)
            search = NB.KnnSearch(qd, k, query_ids=query_ids)      # in order, first_index left to the running count
            for lo in range(0, 200, 63):
                search.update(rd[lo:lo + 63])
            assert search.count == 200 and torch.equal(search.result()[1], one_i) and torch.equal(search.result()[0], one_d)


@pytest.mark.parametrize("nq,n,dim,k", [
    (3, 2100, 3, 5),          # 17 reference tiles: the first size at which groups of 16 lists are folded before the running list
    (3, 131200, 3, 64),       # 1025 tiles: a second pass behind the 1024 a pass may take, 64 groups in the first
    (8192, 1500, 2, 64),      # 8192 x 64 entries a tile: the candidate bytes, not the tile count, cut the call into passes of 10 tiles
])
def test_sizes_where_the_call_folds_in_groups_and_in_passes(nq, n, dim, k):
    from flocoder_amd import neighbors as NB
    q, r = R.exact_case(nq, n, dim)                                # {-1, 0, 1}: ties across tiles, groups and passes go to the lower index
    rows = np.unique(np.concatenate([np.arange(0, nq, 64), [nq - 1]]))
    ids = exclusions(nq, n, 0)
    got_d, got_i = NB.knn(dev(q), dev(r), k, query_ids=dev(ids))
    want_d, want_i = R.knn_ref(q[rows], r, k, query_ids=ids[rows])
    assert torch.equal(got_i.cpu()[rows], torch.from_numpy(want_i)) and torch.equal(got_d.cpu()[rows], torch.from_numpy(want_d.astype(np.float32)))
    rad = R.radii(r[:256])
    got = NB.ball_counts(dev(q), dev(r[:256]), dev(rad)).cpu().numpy()
    assert got[rows].tolist() == R.ball_counts_ref(q[rows], r[:256], rad).tolist()


@pytest.mark.parametrize("dim", [3, 260])
def test_a_pair_has_the_same_bits_whichever_side_is_the_query(dim):
    from flocoder_amd import neighbors as NB
    a, b = R.gauss_case(64, 63, dim)
    d_ab, i_ab = NB.knn(dev(a), dev(b), 63)
    d_ba, i_ba = NB.knn(dev(b), dev(a), 64)
    m_ab = torch.empty(64, 63, device=DEV).scatter_(1, i_ab, d_ab)                     # [a, b]
    m_ba = torch.empty(63, 64, device=DEV).scatter_(1, i_ba, d_ba)                     # [b, a]
    assert torch.equal(m_ab, m_ba.t())


def test_a_query_row_is_the_same_alone_and_inside_a_batch_and_from_call_to_call():
    from flocoder_amd import neighbors as NB
    q, r = R.gauss_case(65, 200, 36)
    qd, rd, rad = dev(q), dev(r), dev(R.radii(r))
    d, i = NB.knn(qd, rd, 5)
    c = NB.ball_counts(qd, rd, rad)
    d2, i2 = NB.knn(qd, rd, 5)
    assert torch.equal(d, d2) and torch.equal(i, i2) and torch.equal(c, NB.ball_counts(qd, rd, rad))
    for row in (0, 37, 64):
        d1, i1 = NB.knn(qd[row:row + 1], rd, 5)
        assert torch.equal(d1[0], d[row]) and torch.equal(i1[0], i[row])
        assert torch.equal(NB.ball_counts(qd[row:row + 1], rd, rad)[0], c[row])


def test_non_finite_rows_sort_last_with_flt_max():
    from flocoder_amd import neighbors as NB
    q, r = R.gauss_case(3, 63, 4)
    r[10, 1], r[20, 3] = np.nan, np.inf
    q[2, 0] = -np.inf
    d, i = NB.knn(dev(q), dev(r), 64)
    assert not torch.isnan(d).any()
    for row in (0, 1):
        assert i[row, 61:].tolist() == [10, 20, -1] and d[row, 61:].tolist() == [FLT_MAX, FLT_MAX, float("inf")]
        assert bool((d[row, :61] < FLT_MAX).all())
    assert i[2].tolist() == list(range(63)) + [-1] and d[2, :63].eq(FLT_MAX).all() and d[2, 63] == float("inf")
    want_d, want_i = R.knn_ref(q, r, 64)
    assert torch.equal(i.cpu(), torch.from_numpy(want_i))
    counts = NB.ball_counts(dev(q), dev(r), torch.full((63,), 1e30, device=DEV))
    assert counts.tolist() == [61, 61, 0]
    counts = NB.ball_counts(dev(q), dev(r), torch.full((63,), float("inf"), device=DEV))
    assert counts.tolist() == [63, 63, 63]


def test_a_copy_of_a_reference_is_at_distance_zero_exactly():
    from flocoder_amd import neighbors as NB
    rng = np.random.default_rng(11)
    r = (rng.standard_normal((130, 4, 32, 32)) * 3).astype(np.float32)                # 4 x 32 x 32 latents: D = 4096
    q = np.stack([r[129], r[5]])
    d, i = NB.knn(dev(q), dev(r), 1)
    assert d.tolist() == [[0.0], [0.0]] and i.tolist() == [[129], [5]]
    d, i = NB.knn(dev(q), dev(r), 2, query_ids=torch.tensor([129, 5], device=DEV))     # the copy kept out: a real distance
    assert bool((d > 0).all()) and 129 not in i[0].tolist() and 5 not in i[1].tolist()


def test_shape_and_argument_errors_surface_as_value_errors():
    from flocoder_amd import _binding as B
    lib = B.lib()
    q, r = torch.zeros(2, 4, device=DEV), torch.zeros(3, 4, device=DEV)
    d, i = torch.full((2, 64), float("inf"), device=DEV), torch.full((2, 64), -1, dtype=torch.int64, device=DEV)
    ws, counts, rad = torch.empty(1 << 16, dtype=torch.uint8, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV), torch.ones(3, device=DEV)
    s = B.current_stream(q.device)
    assert lib.fc_knn_workspace_bytes(2, 3, 64) > 0 and lib.fc_knn_workspace_bytes(2, 0, 1) > 0
    for args in ((2, 3, 0), (2, 3, 65), (0, 3, 1), (2, -1, 1)):
        assert lib.fc_knn_workspace_bytes(*args) == B.FC_E_SHAPE
    for k, dim, n in ((65, 4, 3), (0, 4, 3), (1, 0, 3), (1, 4, -1)):
        rc = lib.fc_knn_update(B.ptr(q), 2, B.ptr(r), n, dim, k, 0, None, B.ptr(d), B.ptr(i), B.ptr(ws), s)
        assert rc == B.FC_E_SHAPE
        with pytest.raises(ValueError):
            B.check(rc)
    assert lib.fc_knn_ball_counts(B.ptr(q), 2, B.ptr(r), 3, 0, B.ptr(rad), 0, None, B.ptr(counts), s) == B.FC_E_SHAPE
    rc = lib.fc_knn_update(None, 2, B.ptr(r), 3, 4, 1, 0, None, B.ptr(d), B.ptr(i), B.ptr(ws), s)
    assert rc == B.FC_E_ARG
    with pytest.raises(ValueError):
        B.check(rc)
    assert lib.fc_knn_update(B.ptr(q), 2, B.ptr(r), 3, 4, 1, 0, None, B.ptr(d), B.ptr(i), None, s) == B.FC_E_ARG
    assert lib.fc_knn_ball_counts(B.ptr(q), 2, B.ptr(r), 3, 4, None, 0, None, B.ptr(counts), s) == B.FC_E_ARG
    assert lib.fc_knn_update(B.ptr(q), 2, B.ptr(r), 0, 4, 1, 0, None, B.ptr(d), B.ptr(i), B.ptr(ws), s) == B.FC_OK     # no references: nothing to do
    torch.cuda.synchronize()
    assert bool((i == -1).all()) and counts.tolist() == [0, 0]
    from flocoder_amd import neighbors as NB
    with pytest.raises(ValueError):
        NB.knn(q, torch.zeros(3, 5, device=DEV), 1)
    with pytest.raises(ValueError):
        NB.ball_counts(q, r, torch.ones(2, device=DEV))


# ---- composition -------------------------------------------------------------------------------------------------------------------
def test_prdc_is_the_metric_assembled_from_the_devices_own_neighbours():
    from flocoder_amd import metrics as M
    from flocoder_amd import neighbors as NB
    real, fake = R.gauss_case(65, 63, 36)
    real, fake, k = dev(real), dev(fake + np.float32(0.5)), 5
    r_real = NB.knn(real, real, k, query_ids=torch.arange(65, device=DEV))[0][:, k - 1].contiguous()
    r_fake = NB.knn(fake, fake, k, query_ids=torch.arange(63, device=DEV))[0][:, k - 1].contiguous()
    in_real, in_fake = NB.ball_counts(fake, real, r_real).cpu().numpy(), NB.ball_counts(real, fake, r_fake).cpu().numpy()
    nearest = NB.knn(real, fake, 1)[0][:, 0]
    want = {"precision": float((in_real > 0).sum()) / 63, "recall": float((in_fake > 0).sum()) / 65, "density": float(in_real.sum()) / (k * 63),
            "coverage": float((nearest <= r_real).sum().item()) / 65}
    got = M.prdc(real, fake, k)
    assert got == want
    assert all(0 < v < 1 for v in got.values()), got                                   # a case that tells the sets apart (fp64: .65 .49 .43 .68)


def test_nearest_in_dataset_over_a_packed_file_equals_knn_on_its_rows(tmp_path):
    from flocoder_amd import neighbors as NB
    from flocoder_amd.data import PackedLatentDataset, pack_latents
    rng = np.random.default_rng(5)
    rows = torch.from_numpy(rng.standard_normal((41, 4, 3, 3)).astype(np.float32))

    class Items(torch.utils.data.Dataset):
        def __len__(self):
            return len(rows)

        def __getitem__(self, idx):
            return rows[idx], idx % 3

    path = tmp_path / "latents.pack"
    pack_latents(Items(), str(path))
    ds = PackedLatentDataset(str(path))
    q = dev(rng.standard_normal((5, 4, 3, 3)).astype(np.float32))
    q[3] = rows[17].to(DEV)
    want_d, want_i = NB.knn(q, rows.to(DEV), 3)
    for chunk_rows in (7, 41, 8192):
        d, i = NB.nearest_in_dataset(q, ds, k=3, chunk_rows=chunk_rows)
        assert torch.equal(d, want_d) and torch.equal(i, want_i)
    assert want_i[3, 0] == 17 and want_d[3, 0] == 0.0                                  # the planted copy is found as a copy
    batches = [(rows[lo:lo + 16], None) for lo in range(0, 41, 16)]
    d, i = NB.nearest_in_dataset(q, batches, k=3)
    assert torch.equal(d, want_d) and torch.equal(i, want_i)
    d, i = NB.nearest_in_dataset(q, ds)
    assert d.shape == (5, 1) and torch.equal(i[:, 0], want_i[:, 0])


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


def test_evaluate_model_with_prdc_k_adds_four_keys_and_changes_nothing_else():
    from flocoder_amd import metrics as M
    from flocoder_amd import sampling as S
    model, codec = small_models()
    g = torch.Generator().manual_seed(7)
    bsz, steps = 7, 2
    target = torch.randn(9, 4, 8, 8, generator=g).to(DEV)
    source = torch.randn(bsz, 4, 8, 8, generator=g).to(DEV)                            # a given start: the two evaluations sample the same latents
    kw = dict(batch_size=bsz, method="rk4", n_steps=steps, is_midi=True, source=source)
    plain = S.evaluate_model(model, codec, 0, target, **kw)
    assert set(plain) == {"sinkhorn", "sinkhorn_px", "mse", "mse_px", "pred_mean", "targ_mean", "pred_std", "targ_std", "pred_px_mean",
                          "targ_px_mean", "pred_px_std", "targ_px_std"} | {k for k in plain if k.startswith("note/")}
    assert not any(k.startswith("prdc") for k in plain)
    got, images = S.evaluate_model(model, codec, 0, target, prdc_k=5, return_images=True, **kw)
    want = dict(plain)
    want.update({f"prdc/{k}": v for k, v in M.prdc(target, images["pred_latents"], 5).items()})
    assert set(got) == set(plain) | {"prdc/precision", "prdc/recall", "prdc/density", "prdc/coverage"}
    for k, v in want.items():
        assert type(got[k]) is float and got[k] == v, (k, got[k], v)
