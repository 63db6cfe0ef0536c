"""Codebook fitting without a GPU: the NumPy definition (flocoder_amd/noise.py, "codebook fitting") against independent statements of the
same algorithms -- scipy's Lloyd iteration, the published EMA lines written directly in torch fp64 -- and the properties of the draws."""
import numpy as np
import pytest
import torch

from flocoder_amd import noise as N


def _lloyd_case(forced_empty):
    g = np.random.default_rng(11 + forced_empty)
    data = g.standard_normal((600, 4))
    init = data[g.permutation(600)[:24]].copy()
    if forced_empty:
        init[5] = 50.0                 # nothing is ever nearest to it: an empty cluster in every iteration
    return data, init


@pytest.mark.parametrize("forced_empty", [0, 1])
def test_lloyd_restatement_agrees_with_scipy(forced_empty):
    """scipy.cluster.vq.kmeans2(minit='matrix') runs ``iter`` Lloyd updates from the given means and keeps an empty cluster's previous
    centroid (it warns); both run in fp64 from the same initial means."""
    from scipy.cluster.vq import kmeans2
    import warnings
    data, init = _lloyd_case(forced_empty)
    means, counts, obj = N.codebook_lloyd(data, init, 15)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref, _ = kmeans2(data, init.copy(), iter=15, minit="matrix")
    assert np.abs(means - ref).max() <= 1e-12
    assert (np.diff(obj) <= 1e-12 * obj[0]).all()                        # Lloyd's property, with the keep-mean rule
    if forced_empty:
        assert counts[5] == 0 and np.array_equal(means[5], init[5])      # kept bit for bit
    else:
        assert counts.sum() == len(data)


def test_ema_restatement_agrees_with_the_published_lines():
    """cluster_size.lerp_(bins, 1 - decay); embed_avg.lerp_(embed_sum, 1 - decay); Laplace smoothing times the total;
    embed = embed_avg / smoothed -- in torch fp64."""
    g = torch.Generator().manual_seed(3)
    k, d, decay, eps = 96, 4, 0.95, 1e-5
    cs = torch.rand(k, generator=g, dtype=torch.float64) * 20
    avg = torch.randn(k, d, generator=g, dtype=torch.float64) * cs[:, None]
    bins = torch.randint(0, 30, (k,), generator=g).double()
    bins[7] = 0
    esum = torch.randn(k, d, generator=g, dtype=torch.float64) * bins[:, None]
    c, a, e = N.codebook_ema(cs.numpy(), avg.numpy(), bins.numpy(), esum.numpy(), decay, dtype=np.float64)
    cs_t, avg_t = cs.clone().lerp_(bins, 1 - decay), avg.clone().lerp_(esum, 1 - decay)
    smoothed = (cs_t + eps) / (cs_t.sum() + k * eps) * cs_t.sum()
    e_t = avg_t / smoothed[:, None]
    for own, ref in ((c, cs_t), (a, avg_t), (e, e_t)):
        assert np.abs(own - ref.numpy()).max() <= 1e-12 * max(1.0, float(ref.abs().max()))
    c32, a32, e32 = N.codebook_ema(cs.numpy(), avg.numpy(), bins.numpy(), esum.numpy(), decay)
    assert c32.dtype == np.float32 and np.abs(e32 - e).max() <= 4 * np.abs(e).max() * 2.0 ** -23


@pytest.mark.parametrize("n", [1, 2, 5, 1031, 4096])
def test_draws_cover_the_range(n):
    p = N.codebook_draws(seed=9, level=2, draw_index=4, n=n, count=n + 7)
    assert p.dtype == np.int64 and np.array_equal(np.sort(p[:n]), np.arange(n))
    assert np.array_equal(p[n:], p[np.arange(n, n + 7) % n])
    assert np.array_equal(N.codebook_draws(9, 2, 4, n, 3), p[:3])        # a slot does not depend on how many are asked for


def test_draws_change_with_seed_level_and_draw_index():
    base = N.codebook_draws(1, 0, 0, 1031)
    for other in (N.codebook_draws(2, 0, 0, 1031), N.codebook_draws(1, 1, 0, 1031), N.codebook_draws(1, 0, 1, 1031),
                  N.codebook_draws(1, 0, 0, 1030, 1031)):
        assert (other != base).mean() > 0.9
    assert np.array_equal(base, N.codebook_draws(1, 0, 0, 1031))
    assert abs(np.corrcoef(base[:-1], base[1:])[0, 1]) < 0.1             # neighbouring slots are not neighbours in the data
    with pytest.raises(ValueError):
        N.codebook_draws(0, 0, 0, (1 << 24) + 1, 4)


def test_expiry_takes_the_drawn_rows():
    g = np.random.default_rng(5)
    k, d, n = 32, 3, 257
    cs = g.uniform(0, 4, k).astype(np.float32)
    embed, r = g.standard_normal((k, d)).astype(np.float32), g.standard_normal((n, d)).astype(np.float32)
    avg = embed * cs[:, None]
    c2, a2, e2, dead = N.codebook_expire(cs, avg, embed, r, 2, seed=3, level=1, draw_index=6)
    assert np.array_equal(dead, np.flatnonzero(cs < 2)) and 0 < dead.size < k
    assert np.array_equal(e2[dead], r[N.codebook_draws(3, 1, 6, n, dead.size)])
    assert (c2[dead] == 2).all() and np.array_equal(a2[dead], e2[dead] * np.float32(2))
    alive = np.setdiff1d(np.arange(k), dead)
    assert np.array_equal(e2[alive], embed[alive]) and np.array_equal(c2[alive], cs[alive])
    assert N.codebook_expire(cs, avg, embed, r, 0, 3, 1, 6)[3].size == 0


def test_state_dict_keeps_four_keys_per_level_and_the_constructor_its_defaults():
    from flocoder_amd.codecs import VQVAE, ResidualVQ
    q = ResidualVQ(4, 96, 3)
    assert (q.decay, q.commitment_weight, q.kmeans_init, q.kmeans_iters, q.threshold_ema_dead_code, q.seed, q.draw_index) == \
        (0.95, 0.25, True, 15, 2.0, 0, 0)
    assert len(q.state_dict()) == 4 * 3 and not any("seed" in k or "draw" in k for k in q.state_dict())
    m = VQVAE(in_channels=1, hidden_channels=32, num_downsamples=4, internal_dim=32, vq_embedding_dim=4, vq_num_embeddings=64,
              codebook_levels=3, commitment_weight=0.5)
    vqk = [k for k in m.state_dict() if k.startswith("vq.")]
    assert len(vqk) == 4 * 3 and m.vq.commitment_weight == 0.5 and m.vq.threshold_ema_dead_code == 2.0
    with pytest.raises(RuntimeError, match="no CPU path"):
        q.train()(torch.zeros(8, 4))
    with pytest.raises(NotImplementedError, match="uninitialised"):
        q.eval()(torch.zeros(8, 4))
