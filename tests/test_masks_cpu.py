"""The counter-based inpainting masks on the host: ``flocoder_amd.noise.mask_field`` against what the reference's generator drew
(tests/golden/g13_masks.npz, tools/make_mask_golden.py: coverage of every mask and the per-pixel frequency image of 4000 masks per
type at 128 x 128), and the field's own contract (type frequencies, forced types, batch independence, key separation, the committed
sine / cosine table, the accepted sizes).  No bound here is tuned: each is the inequality its docstring names."""
import os

import numpy as np
import pytest

from flocoder_amd import noise as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_masks.npz")
SEED, N_IDS, SIZE = 1300, 4000, (128, 128)
ALPHA, Z_PIXEL = 1e-6, 5.5


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    assert int(g["n"]) == N_IDS and [str(t) for t in g["types"]] == ["brush", "rectangles", "noise"]
    return g


@pytest.fixture(scope="module")
def ours():
    """type name -> bool [4000, 128, 128]: the restatement's masks of ids 0 .. 3999, computed once."""
    return {t: N.mask_field(SEED, np.arange(N_IDS), SIZE, mask_type=t)[:, 0] != 0 for t in ("brush", "rectangles", "noise")}


def ks_distance(a, b):
    a, b = np.sort(a), np.sort(b)
    pts = np.concatenate([a, b])
    return float(np.abs(np.searchsorted(a, pts, side="right") / a.size - np.searchsorted(b, pts, side="right") / b.size).max())


@pytest.mark.parametrize("k,name", list(enumerate(("brush", "rectangles", "noise"))))
def test_coverage_distribution_matches_reference(golden, ours, k, name):
    """Two-sample Kolmogorov-Smirnov: D <= sqrt(-ln(alpha/2)/2) sqrt((n+m)/(n m)), alpha = 1e-6, n = m = 4000: 0.060."""
    n = m = N_IDS
    bound = np.sqrt(-np.log(ALPHA / 2) / 2) * np.sqrt((n + m) / (n * m))
    assert abs(bound - 0.060) < 5e-4
    cov = ours[name].reshape(N_IDS, -1).sum(axis=1)
    d = ks_distance(cov, golden["coverage"][k].astype(np.int64))
    print(name, "KS", d, "bound", bound, "mean coverage", cov.mean() / 16384, golden["coverage"][k].mean() / 16384)
    assert d <= bound


@pytest.mark.parametrize("k,name", [(0, "brush"), (1, "rectangles")])
def test_pixel_frequencies_match_reference(golden, ours, k, name):
    """Every pixel: |p - q| <= 5.5 sqrt(max(pbar (1 - pbar), 1/N) 2/N), pbar pooled; two-sided z = 5.5 over 16384 pixels is a family-wise
    false-alarm rate below 1e-3.  (A transposed mask misses this by a factor of eight.)"""
    p, q = ours[name].mean(axis=0), golden["counts"][k] / N_IDS
    pbar = (p + q) / 2
    z = np.abs(p - q) / np.sqrt(np.maximum(pbar * (1 - pbar), 1.0 / N_IDS) * 2.0 / N_IDS)
    print(name, "largest z", z.max())
    assert z.max() <= Z_PIXEL
    zt = np.abs(p.T - q) / np.sqrt(np.maximum(pbar * (1 - pbar), 1.0 / N_IDS) * 2.0 / N_IDS)
    assert zt.max() > Z_PIXEL                       # the check does tell the two axes apart


@pytest.mark.parametrize("choices,p", [(N.MASK_TYPES, N.MASK_DEFAULT_P), (("rectangles", "brush", "nothing"), (0.25, 0.6, 0.15))])
def test_type_frequencies(choices, p):
    n = 20000
    t = N.mask_types(SEED, np.arange(n), choices, p)
    for name, pk in zip(choices, p):
        count = int((t == N.MASK_TYPES.index(name)).sum())
        assert abs(count - n * pk) <= 5 * np.sqrt(n * pk * (1 - pk)), (name, count)
    assert set(np.unique(t)) <= {N.MASK_TYPES.index(c) for c in choices}
    m, t2 = N.mask_field(SEED, np.arange(40), (16, 16), choices, p, return_types=True)
    assert np.array_equal(t2, t[:40]) and t2.dtype == np.int32 and m.dtype == np.float32 and m.shape == (40, 1, 16, 16)


def test_forced_types(ours):
    ids = np.arange(5)
    assert (N.mask_field(SEED, ids, (32, 64), mask_type="total") == 1).all()
    assert (N.mask_field(SEED, ids, (32, 64), mask_type="nothing") == 0).all()
    px = ours["noise"].size
    assert abs(ours["noise"].mean() - 0.3) <= 5 * np.sqrt(0.3 * 0.7 / px)
    for t in ("brush", "rectangles", "noise"):
        assert set(np.unique(N.mask_field(SEED, ids, (32, 64), mask_type=t))) <= {0.0, 1.0}
    with pytest.raises(ValueError):
        N.mask_field(SEED, ids, (32, 64), mask_type="cv2")
    with pytest.raises(ValueError):
        N.mask_field(SEED, ids, (32, 64), choices=("total", "brush"), p=(0.5, 0.6))


def test_batch_independence_and_keys():
    ids = np.array([5, -3, (1 << 32) + 7, 0, 123456789012, 17, 2, 9], dtype=np.int64)
    seed = (1 << 32) + 99
    whole, types = N.mask_field(seed, ids, (48, 40), return_types=True)
    perm = np.array([3, 7, 0, 5, 1, 6, 2, 4])
    shuffled, types_p = N.mask_field(seed, ids[perm], (48, 40), return_types=True)
    assert np.array_equal(shuffled, whole[perm]) and np.array_equal(types_p, types[perm])
    for b in range(ids.size):
        one, t1 = N.mask_field(seed, ids[b:b + 1], (48, 40), return_types=True)
        assert np.array_equal(one[0], whole[b]) and t1[0] == types[b]
    for t in ("brush", "rectangles", "noise"):                                    # and with every generator forced
        whole = N.mask_field(seed, ids, (48, 40), mask_type=t)
        assert np.array_equal(N.mask_field(seed, ids[perm], (48, 40), mask_type=t), whole[perm])
        assert np.array_equal(N.mask_field(seed, ids[2:3], (48, 40), mask_type=t)[0], whole[2])
        assert not np.array_equal(N.mask_field(seed + 1, ids, (48, 40), mask_type=t), whole)
    # the mask words of a seed are neither the SDE field's nor the probe field's of the same seed and ids
    j = np.arange(16)
    mw = N.mask_words(seed, ids, 1, j).astype(np.uint32)
    sde = N.field_words(seed, 1, ids, 64)
    probe = N.field_words((seed + N.PROBE_KEY_OFFSET) & 0xffffffffffffffff, 1, ids, 64)
    assert mw.shape == sde.shape == probe.shape
    assert not (mw == sde).all(axis=-1).any() and not (mw == probe).all(axis=-1).any()
    assert not np.array_equal(mw, N.mask_words(seed + 1, ids, 1, j).astype(np.uint32))
    assert N.MASK_KEY_OFFSET not in (0, N.PROBE_KEY_OFFSET)


def test_trig_table_is_its_formula():
    tab = N.mask_trig_table()
    assert tab.shape == (4096,) and np.array_equal(tab, N.mask_trig_formula())
    a = np.arange(4096)
    sine = np.rint(np.sin(a * (2 * np.pi / 4096)) * (0.7 * 65536)).astype(np.int64)
    assert np.array_equal(tab[(a - 1024) & 4095], sine)                           # the sine is the entry a quarter turn back
    assert tab[0] == 45875 and tab[1024] == 0 and tab[2048] == -45875


def test_sizes():
    for size in ((16, 16), (32, 64)):
        for t in ("", "brush", "rectangles", "noise"):
            m = N.mask_field(SEED, np.arange(6), size, mask_type=t)
            assert m.shape == (6, 1, *size)
    assert N.mask_field(SEED, np.arange(64), (16, 16), mask_type="brush").any()
    for size in ((15, 16), (16, 15), (1025, 16), (16, 1025)):
        with pytest.raises(ValueError):
            N.mask_field(SEED, [0], size)


def test_public_numpy_surface():
    """generate_mask / generate_mask_batch with to_tensor=False are the NumPy form under upstream's names; tensors on the CPU raise."""
    from flocoder_amd import inpainting as I
    m, name = I.generate_mask((32, 64), to_tensor=False, seed=3, sample_id=11, return_type=True)
    ref, t = N.mask_field(3, [11], (32, 64), return_types=True)
    assert m.shape == (32, 64) and np.array_equal(m, ref[0, 0]) and name == N.MASK_TYPES[int(t[0])]
    tiled = I.generate_mask_batch((16, 16), 4, to_tensor=False, seed=3, mask_type="brush")
    assert tiled.shape == (4, 16, 16) and all(np.array_equal(tiled[0], tiled[b]) for b in range(4))
    uniq = I.generate_mask_batch((16, 16), 4, unique_masks=True, to_tensor=False, seed=3, mask_type="brush", sample_ids=[4, 5, 6, 7])
    assert np.array_equal(uniq, N.mask_field(3, [4, 5, 6, 7], (16, 16), mask_type="brush")[:, 0])
    with pytest.raises(RuntimeError):
        I.generate_mask((16, 16), device="cpu")
    import torch
    with pytest.raises(RuntimeError):
        I.create_inpainting_triplet(torch.zeros(1, 1, 16, 16), codec=None)
