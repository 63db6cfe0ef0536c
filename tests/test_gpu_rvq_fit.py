"""Codebook fitting on the device (csrc/rvq_train.hip: fc_codebook_draws, fc_rvq_seed_codes, fc_rvq_kmeans, fc_rvq_train_step;
codecs.ResidualVQ in training mode, VQVAE.fit_codebooks) against the fp64 restatement tests/rvq_fit_ref.py.

Shapes (D, K, L, N): (4,96,4), (1,32,2), (3,64,3) at N = 1031 -- more than one 256-thread workgroup and a ragged last one -- and
(16,256,4), exactly 64 KB of codebooks, at N = 16 K + 7 = 4103: checked in NumPy (Gaussian data, codes seeded by the draws, fifteen
Lloyd iterations per level), the index rule leaves out at most 2 of its 4103 vectors in any iteration, against a cap of 41, and at
most 1 of 1031 at the other shapes.  The k-means test also runs (16,256,4) at N = 1031, four vectors per code: 22 to 49 clusters of
its deeper levels are empty without being forced and the same check left out none of the 1031, so the keep-mean branch is met there
as it arises.

INDEX RULE (that of test_rvq_quantize_alone_vs_fp64): indices are compared on the vectors whose best and second-best fp64 distances
differ by at least 1e-5 relative; at most 1 % may be left out.  The restatement is always handed the device's own current codebooks and
indices, one iteration at a time, so one rounding flip cannot cascade.

ACCUMULATION BOUND: the sums are 64-bit integer atomics on rint(r 2^s), s = 38 - e with 2^e the power of two above
M = max|z| + sum_{l < last} max|E_l|.  One conversion errs by at most 2^(e-39) <= M 2^-38, a sum over n_k vectors by n_k 2^(e-39), a
mean by 2^(e-39); integer addition adds nothing and does not depend on the order.  embed_avg carries (1 - decay) n_k 2^(e-39), the
codebook that divided by the smoothed cluster size, each next to one fp32 ulp of the restatement's value (a stored value may round the
other way).  The commitment sum is fp64 in a fixed order: against another fp64 order it may differ by N D 2^-52 relative.
Largest measured fraction of these tolerances: embed_avg 0.000 and codebook 0.000 (every value bit-equal to the restatement's), loss
0.476, k-means means 0.500 (printed by -s)."""
import numpy as np
import pytest
import torch

import rvq_fit_ref as R
from flocoder_amd import noise as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(4, 96, 4, 1031), (1, 32, 2, 1031), (3, 64, 3, 1031), (16, 256, 4, 4103)]
DECAY, CW = 0.95, 0.25


def _lib():
    from flocoder_amd import _binding as B
    return B, B.lib()


def _data(D, K, L, n):
    g = torch.Generator().manual_seed(100 * D + L)
    z = torch.randn(n, D, generator=g)
    cbs = torch.stack([torch.randn(K, D, generator=g) * 0.5 ** l for l in range(L)])
    cs = torch.rand(L, K, generator=g) * 4                                  # some below the threshold 2, some above
    return z, cbs, cs, cbs * cs[..., None]


def _zt(z):
    return z.t().contiguous().to(DEV)                                       # the boundary layout [B = 1, D, hw = N]


def _ws(n, D, K, L):
    B, lib = _lib()
    nbytes = lib.fc_rvq_train_workspace_bytes(1, n, D, K, L)
    assert nbytes > 0
    return torch.empty(nbytes, dtype=torch.uint8, device=DEV), nbytes


def _quantize(zt, cb):
    B, lib = _lib()
    L, K, D = cb.shape
    n = zt.shape[1]
    zq = torch.full_like(zt, float("nan"))
    idx = torch.full((n, L), -1, dtype=torch.int64, device=DEV)
    B.check(lib.fc_rvq_quantize(B.ptr(zt), B.ptr(cb), B.ptr(zq), B.ptr(idx), 1, D, n, K, L, B.current_stream(zt.device)))
    return zq, idx


def _step(z, cbs, cs, avg, decay=DECAY, thr=0.0, seed=3, draw=5):
    """-> dict of CPU tensors: the updated buffers, z_q, indices, losses, expired; plus fc_rvq_quantize's outputs on the input codebooks."""
    B, lib = _lib()
    L, K, D = cbs.shape
    n = z.shape[0]
    zt, cb, c, a = _zt(z), cbs.clone().to(DEV), cs.clone().to(DEV), avg.clone().to(DEV)
    ref_q, ref_idx = _quantize(zt, cb)
    ws, nbytes = _ws(n, D, K, L)
    zq, idx = torch.full_like(zt, float("nan")), torch.full((n, L), -1, dtype=torch.int64, device=DEV)
    losses, expired = torch.full((L,), float("nan"), device=DEV), torch.full((L,), -1, dtype=torch.int32, device=DEV)
    B.check(lib.fc_rvq_train_step(B.ptr(zt), B.ptr(cb), B.ptr(c), B.ptr(a), B.ptr(zq), B.ptr(idx), B.ptr(losses), B.ptr(expired), 1, D, n, K, L,
                                  decay, CW, thr, seed, draw, B.ptr(ws), nbytes, B.current_stream(zt.device)))
    torch.cuda.synchronize()
    return dict(cb=cb.cpu(), cs=c.cpu(), avg=a.cpu(), zq=zq.cpu(), idx=idx.cpu(), losses=losses.cpu(), expired=expired.cpu(),
                ref_q=ref_q.cpu(), ref_idx=ref_idx.cpu())


def _check_indices(r, means, idx, tag):
    """The index rule for one level: r fp32 [N, D] the residuals the device assigned, means its codebook, idx its indices."""
    ref, ok = R.sure(r, means)
    left = int((~ok).sum())
    print(f"[{tag}] {left} of {len(r)} vectors left out, mismatches among the rest {int((ref[ok] != idx[ok]).sum())}")
    assert left <= len(r) // 100
    assert np.array_equal(ref[ok], idx[ok])


def test_draws_equal_the_host_form():
    B, lib = _lib()
    for seed, level, draw, n, count in [(0, 0, 0, 1031, 1031), (2 ** 63 + 5, 3, 17, 4096, 5000), (7, 1, 2 ** 32 - 1, 1, 4), (7, 1, 0, 2, 5),
                                        (11, 2, 9, 5, 12), (11, 0, 1, 1 << 24, 3000), (11, 0, 1, (1 << 23) + 1, 3000)]:
        out = torch.full((count,), -1, dtype=torch.int64, device=DEV)
        B.check(lib.fc_codebook_draws(B.ptr(out), seed, level, draw, n, count, B.current_stream(out.device)))
        assert np.array_equal(out.cpu().numpy(), N.codebook_draws(seed, level, draw, n, count)), (seed, level, draw, n)


@pytest.mark.parametrize("D,K,L,n", SHAPES)
def test_training_step_from_given_codebooks(D, K, L, n):
    z, cbs, cs, avg = _data(D, K, L, n)
    out = _step(z, cbs, cs, avg, thr=0.0)
    assert torch.equal(out["idx"], out["ref_idx"]) and torch.equal(out["zq"], out["ref_q"])         # fc_rvq_quantize's, bit for bit
    assert int(out["expired"].abs().sum()) == 0
    zn, cn, idx = z.numpy(), cbs.numpy(), out["idx"].numpy()
    ref = R.train_step(zn, cn, cs.numpy(), avg.numpy(), idx, DECAY, CW, 0.0, 3, 5)
    exact = _step(z, cbs, torch.zeros_like(cs), torch.zeros_like(avg), decay=0.0)                   # decay 0: cluster_size <- the counts
    frac = dict(avg=0.0, embed=0.0, loss=0.0)
    for l, want in enumerate(ref):
        _check_indices(R.residuals(zn, cn, idx, l), cn[l], idx[:, l], f"step D={D} K={K} level {l}")
        assert np.array_equal(exact["cs"][l].numpy(), want["counts"].astype(np.float32)) and want["counts"].sum() == n
        assert np.array_equal(out["cs"][l].numpy(), want["cs"])                                      # bit for bit
        for key, got, tol in (("avg", out["avg"][l], want["tol_avg"]), ("embed", out["cb"][l], want["tol_embed"])):
            err = np.abs(got.numpy().astype(np.float64) - want[key].astype(np.float64)) / tol
            frac[key] = max(frac[key], float(err.max()))
        frac["loss"] = max(frac["loss"], abs(float(out["losses"][l]) - want["loss"]) / want["tol_loss"])
    print(f"[step D={D} K={K} L={L} N={n}] largest fraction of the tolerance: " + ", ".join(f"{k} {v:.3f}" for k, v in frac.items()))
    assert max(frac.values()) <= 1.0


@pytest.mark.parametrize("D,K,L,n", SHAPES)
def test_expiry(D, K, L, n):
    z, cbs, cs, avg = _data(D, K, L, n)
    out = _step(z, cbs, cs, avg, thr=2.0, seed=21, draw=4)
    assert torch.equal(out["idx"], out["ref_idx"]) and torch.equal(out["zq"], out["ref_q"])
    zn, cn, idx = z.numpy(), cbs.numpy(), out["idx"].numpy()
    ref = R.train_step(zn, cn, cs.numpy(), avg.numpy(), idx, DECAY, CW, 2.0, 21, 4)
    total = 0
    for l, want in enumerate(ref):
        dead = want["dead"]
        alive = np.setdiff1d(np.arange(K), dead)
        total += dead.size
        assert int(out["expired"][l]) == dead.size
        got_cs, got_cb, got_avg = out["cs"][l].numpy(), out["cb"][l].numpy(), out["avg"][l].numpy()
        assert np.array_equal(np.flatnonzero(got_cs != want["cs"]), dead[want["cs"][dead] != 2.0])   # the replaced set, exactly
        assert np.array_equal(got_cb[dead], want["embed2"][dead])                                    # the drawn fp32 residuals, bit for bit
        assert (got_cs[dead] == 2.0).all() and np.array_equal(got_avg[dead], want["avg2"][dead])
        assert np.array_equal(got_cs[alive], want["cs"][alive])
        assert (np.abs(got_cb[alive].astype(np.float64) - want["embed"][alive]) <= want["tol_embed"][alive]).all()
        assert (np.abs(got_avg[alive].astype(np.float64) - want["avg"][alive]) <= want["tol_avg"][alive]).all()
    print(f"[expiry D={D} K={K} L={L}] replaced {total} of {L * K} codes")
    assert 0 < total < L * K
    none = _step(z, cbs, cs, avg, thr=0.0, seed=21, draw=4)
    assert int(none["expired"].abs().sum()) == 0
    for l, want in enumerate(ref):
        assert np.array_equal(none["cs"][l].numpy(), want["cs"])                                     # nothing set to a threshold


def _kmeans(zt, cb, level, iters, ws, nbytes, stats=False, objective=False):
    B, lib = _lib()
    L, K, D = cb.shape
    cs = torch.full((K,), float("nan"), device=DEV) if stats else None
    ea = torch.full((K, D), float("nan"), device=DEV) if stats else None
    obj = torch.full((max(iters, 1),), float("nan"), dtype=torch.float64, device=DEV) if objective else None
    B.check(lib.fc_rvq_kmeans(B.ptr(zt), B.ptr(cb), 1, D, zt.shape[1], K, L, level, iters, B.ptr(cs), B.ptr(ea), B.ptr(obj), B.ptr(ws), nbytes,
                              B.current_stream(zt.device)))
    return cs, ea, obj


@pytest.mark.parametrize("D,K,L,n", SHAPES + [(16, 256, 4, 1031)])
def test_kmeans(D, K, L, n):
    """Level after level, as the initialisation runs: seed the level's codes, then fifteen single iterations checked one by one against
    the restatement (code 3 is moved far away first, so every iteration has an empty cluster), and the same fifteen in one call."""
    B, lib = _lib()
    z, cbs, _, _ = _data(D, K, L, n)
    zn, zt = z.numpy(), _zt(z)
    cb = cbs.clone().to(DEV)
    ws, nbytes = _ws(n, D, K, L)
    frac, n_empty = 0.0, 0
    for l in range(L):
        B.check(lib.fc_rvq_seed_codes(B.ptr(zt), B.ptr(cb), 1, D, n, K, L, l, 13, 2, B.current_stream(zt.device)))
        _, idx = _quantize(zt, cb)
        r = R.residuals(zn, cb.cpu().numpy(), idx.cpu().numpy(), l)
        assert np.array_equal(cb[l].cpu().numpy(), r[N.codebook_draws(13, l, 2, n, K)])              # the drawn residuals, bit for bit
        cb[l, 3] = 50.0
        start = cb.clone()
        cs15, ea15, obj15 = _kmeans(zt, cb, l, 15, ws, nbytes, stats=True, objective=True)
        many = cb.clone()
        cb.copy_(start)
        unit, objs = R.fix_unit(zn, cb.cpu().numpy(), l), []
        for it in range(15):
            before = cb.cpu().numpy()
            idx = _quantize(zt, cb)[1].cpu().numpy()[:, l]                  # the same search: the iteration's own indices
            cs1, ea1, obj1 = _kmeans(zt, cb, l, 1, ws, nbytes, stats=True, objective=True)
            after = cb.cpu().numpy()
            _check_indices(r, before[l], idx, f"kmeans D={D} K={K} level {l} iteration {it}")
            want, counts, obj = R.lloyd_update(r, before[l], idx)
            empty = counts == 0
            n_empty += int(empty.sum())
            assert empty[3] and np.array_equal(after[l][empty], before[l][empty])                    # kept bit for bit
            assert np.array_equal(after[:l], before[:l]) and np.array_equal(after[l + 1:], before[l + 1:])
            frac = max(frac, float((np.abs(after[l].astype(np.float64) - want) / (R.ulp32(want) + unit)).max()))
            assert abs(float(obj1[0]) - obj) <= 1e-12 * obj
            assert np.array_equal(cs1.cpu().numpy(), counts.astype(np.float32))
            assert np.array_equal(ea1.cpu().numpy(), after[l] * counts.astype(np.float32)[:, None])
            objs.append(float(obj1[0]))
        assert torch.equal(cb, many), "fifteen iterations in one call != fifteen calls of one"
        assert torch.equal(cs15, cs1) and torch.equal(ea15, ea1) and np.array_equal(obj15.cpu().numpy(), np.array(objs))
        assert all(b <= a * (1 + 1e-6) for a, b in zip(objs, objs[1:])) and objs[-1] < objs[0]
    print(f"[kmeans D={D} K={K} L={L} N={n}] largest fraction of the tolerance {frac:.3f}; empty clusters met {n_empty}")
    assert frac <= 1.0
    zero = _kmeans(zt, cb, 0, 0, ws, nbytes, stats=True)
    assert torch.equal(cb, many) and float(zero[0].abs().sum()) == 0.0 and float(zero[1].abs().sum()) == 0.0


def _buffers(q):
    return {k: v.detach().cpu().clone() for k, v in q.state_dict().items()}


def _fit(seed, z):
    from flocoder_amd.codecs import ResidualVQ
    q = ResidualVQ(4, 96, 4, seed=seed).to(DEV).train()
    out = q.quantize_nchw(z)
    return q, out


def test_end_to_end_residual_vq():
    from flocoder_amd.codecs import ResidualVQ
    g = torch.Generator().manual_seed(8)
    z = torch.randn(5, 4, 16, 16, generator=g).to(DEV)                      # N = 1280 over five samples: the NCHW addressing
    z2 = torch.randn(5, 4, 16, 16, generator=g).to(DEV)
    q, (zq, idx, losses) = _fit(5, z)
    assert all(bool(l._codebook.initted) for l in q.layers) and q.draw_index == 1
    assert losses.shape == (1, 4) and bool((losses > 0).all()) and not zq.requires_grad and q.last_expired.shape == (4,)
    assert bool((losses[0, 1:] < losses[0, :-1]).all())                     # every level quantises a smaller residual
    q.eval()
    ezq, eidx, eloss = q.quantize_nchw(z)
    rq, ridx = _quantize(z.reshape(5, 4, 256).permute(1, 0, 2).reshape(4, 1280).contiguous(), q.codebooks.contiguous())
    assert float(eloss.abs().sum()) == 0.0 and q.draw_index == 1
    flat = lambda t: t.reshape(5, 4, 256).permute(1, 0, 2).reshape(4, 1280)
    assert torch.equal(flat(ezq), rq) and torch.equal(eidx, ridx)
    zf = flat(z).t().cpu().numpy()
    first = zf[N.codebook_draws(5, 0, 0, 1280, 96)]                          # level 0's drawn initial codes
    err = lambda codes: float(N.codebook_assign(zf, codes)[1].mean())
    e0, e1 = err(first), err(q.codebooks[0].cpu().numpy())
    print(f"[fit] level-0 mean squared error: drawn codes {e0:.4f}, fitted {e1:.4f}")
    assert e1 < e0
    same, _ = _fit(5, z)
    other, _ = _fit(6, z)
    a, b, c = _buffers(q), _buffers(same), _buffers(other)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert any(not torch.equal(a[k], c[k]) for k in a if k.endswith("embed"))
    fresh = ResidualVQ(4, 96, 4, seed=5).to(DEV)
    fresh.load_state_dict(q.state_dict())
    fresh.draw_index = q.draw_index
    o1, o2 = q.train().quantize_nchw(z2), fresh.train().quantize_nchw(z2)
    assert all(torch.equal(u, v) for u, v in zip(o1, o2))
    a, b = _buffers(q), _buffers(fresh)
    assert all(torch.equal(a[k], b[k]) for k in a) and q.draw_index == 2
    flat_in = z2.permute(0, 2, 3, 1).reshape(-1, 4)                          # the `.vq(flat)` protocol in training mode
    fq, fidx, floss = q(flat_in)
    assert fq.shape == flat_in.shape and fidx.shape == (1280, 4) and floss.shape == (1, 4) and q.draw_index == 3


def test_vqvae_fit_codebooks():
    from conftest import load_golden
    from oracle.synth import synth_state_dict
    from flocoder_amd.codecs import VQVAE
    m = VQVAE(vq_num_embeddings=64, codebook_levels=3, in_channels=1, hidden_channels=32, num_downsamples=4, internal_dim=32,
              vq_embedding_dim=4).eval()                                     # the gray_nd4_small shape of test_gpu_vqvae.py
    m.load_state_dict(synth_state_dict(load_golden("g9_vqvae")["gray_nd4_small_shapes"], 9), strict=False)
    m = m.to(DEV)
    g = torch.Generator().manual_seed(2)
    batches = [torch.rand(2, 1, 128, 128, generator=g).to(DEV), (torch.rand(2, 1, 128, 128, generator=g).to(DEV), None)]
    with pytest.raises(NotImplementedError):
        m(batches[0])                                                        # nothing fitted, nothing loaded
    weights = m.get_parameter("encoder.0.conv1.weight").clone()
    losses, expired = m.fit_codebooks(batches, epochs=2)
    assert losses.shape == (4, 3) and expired.shape == (4, 3) and losses.is_cuda and expired.is_cuda and not m.training and not m.vq.training
    assert bool(torch.isfinite(losses).all()) and m.vq.draw_index == 4
    assert torch.equal(weights, m.get_parameter("encoder.0.conv1.weight"))
    recon, closs = m(batches[0])
    assert recon.shape == batches[0].shape and bool(torch.isfinite(recon).all()) and float(closs) == 0.0
    before = m.vq.codebooks.clone()
    m.fit_codebooks(batches[:1], reset=True)
    assert m.vq.draw_index == 5 and not torch.equal(before, m.vq.codebooks) and not m.training
    with pytest.raises(NotImplementedError):
        m.train()(batches[0])                                                # codec training through the encoder stays out
    m.eval()


def test_protocol():
    from flocoder_amd.codecs import ResidualVQ
    B, lib = _lib()
    q = ResidualVQ(4, 96, 4).to(DEV)
    with pytest.raises(NotImplementedError, match="uninitialised"):
        q.eval().quantize_nchw(torch.zeros(1, 4, 8, 8, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU path"):
        q.train().quantize_nchw(torch.zeros(1, 4, 8, 8))
    assert q.draw_index == 0 and not any(bool(l._codebook.initted) for l in q.layers)
    with pytest.raises(ValueError, match="embedding dim must be 1..16"):
        ResidualVQ(17, 8, 1).to(DEV).train().quantize_nchw(torch.zeros(1, 17, 4, 4, device=DEV))
    with pytest.raises(ValueError, match="codebooks exceed 64 KB"):
        ResidualVQ(16, 257, 4).to(DEV).train().quantize_nchw(torch.zeros(1, 16, 4, 4, device=DEV))
    for D, K, L in [(17, 8, 1), (16, 257, 4)]:
        assert lib.fc_rvq_train_workspace_bytes(1, 16, D, K, L) == 0
        t = torch.zeros(L * K * D + 64, device=DEV)
        i64, i32 = torch.zeros(16 * L, dtype=torch.int64, device=DEV), torch.zeros(L, dtype=torch.int32, device=DEV)
        s = B.current_stream(t.device)
        assert lib.fc_rvq_train_step(B.ptr(t), B.ptr(t), B.ptr(t), B.ptr(t), B.ptr(t), B.ptr(i64), B.ptr(t), B.ptr(i32), 1, D, 16, K, L, DECAY, CW,
                                     2.0, 0, 0, B.ptr(t), 64, s) == B.FC_E_SHAPE
        assert lib.fc_rvq_kmeans(B.ptr(t), B.ptr(t), 1, D, 16, K, L, 0, 1, None, None, None, B.ptr(t), 64, s) == B.FC_E_SHAPE
        assert lib.fc_rvq_seed_codes(B.ptr(t), B.ptr(t), 1, D, 16, K, L, 0, 0, 0, s) == B.FC_E_SHAPE
    assert lib.fc_rvq_train_workspace_bytes(1 << 12, (1 << 12) + 1, 4, 96, 4) == 0       # more than 2^24 vectors
    torch.cuda.synchronize()
