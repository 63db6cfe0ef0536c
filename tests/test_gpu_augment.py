"""Pre-encoding augmentation on the GPU (fc_augment_images / fc_augment_midi, csrc/augment.hip) against its NumPy definitions
``flocoder_amd.noise.augment_image_field`` (every output pixel, within a derived rounding bound: the choice of source pixels is integer
arithmetic on both sides, nothing is left out) and ``augment_midi_field`` (bit-equal), its independence of row, batch and stream, the C
ABI's argument checks, and the whole ``AugmentedBatches`` -> ``process_dataset(packed=True)`` -> ``PackedLatentDataset`` path.

The image bound.  The device forms A = sum_y ny (sum_x nx p) in fp32 with integer numerators nx, ny < 2^15 and bytes p: the products
nx p are exact, each of the tx - 1 inner and ty - 1 outer additions and each product ny r rounds once, and every term is non-negative,
so |A - exact| <= (tx + ty) u A with u = 2^-24.  Then, on a value of at most M = max(1, |fill std + mean|) in units of a byte / 255:
the fill byte's rounding to fp32, its product with the weight that fell outside the source and the addition (3 u), the two reciprocals
1 / N (conversion and division, 2 u each), their product, the scaling and / 255 (3 u): 10 u.  The subtraction of the mean and the
division by std round once each, on values of at most M + |mean| and (M + |mean|) / std.  In all
    |err| <= (tx + ty + 12) u (M + |mean|) / std
which is the issue's c n 2^-24 / std with n = tx + ty taps (the sums are separable: the error grows with the sum of the two tap counts,
not their product) and c = (1 + 12 / n) (M + |mean|), the 12 being the fixed operations that do not scale with the taps.  tx, ty are
the largest tap counts among the call's boxes.  The definition is fp64: its own error is 2^-29 of this."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden
from flocoder_amd import noise as N
from oracle.synth import synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = (1 << 32) + 2718
U = 2.0 ** -24


def synthetic(h, w, channels=3, k=0):
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([(x * 255 // (w - 1) + 7 * k) % 256, y * 255 // (h - 1), ((x + y + k) % 2) * 255], axis=-1).astype(np.uint8)
    return a if channels == 3 else (a[:, :, 2:3] // 2 + a[:, :, 0:1] // 2).astype(np.uint8)


def ids_for(bsz):
    ids = np.arange(bsz, dtype=np.int64) * 3 + 1
    ids[0] = -5
    ids[-1] = (1 << 32) + 12345
    return ids


SOURCES = [synthetic(96, 96), synthetic(53, 37, 1, 1), synthetic(150, 200, 3, 2), synthetic(768, 1024, 3, 3)]


@pytest.fixture(scope="module")
def pool():
    from flocoder_amd.augment import ImagePool
    p = ImagePool.from_arrays(SOURCES, labels=[0, 1, 2, 3], device=DEV)
    assert len(p) == 4 and p.nbytes >= sum(a.size for a in SOURCES) and p.buffer.dtype == torch.uint8 and p.buffer.is_cuda
    return p


def forced(params, bsz):
    """The first samples at the angle's ends and at zero, and both flips whatever the draws."""
    k = min(3, bsz)
    params["angle"][:k] = (-15.0, 0.0, 15.0)[:k]
    params["flip"][:bsz:2] = True
    params["flip"][1:bsz:2] = False
    return params


def image_bound(params, size, mean, std, fill):
    taps = 0
    for bx, by, bw, bh, side in zip(*(params[k] for k in ("box_left", "box_top", "box_w", "box_h", "crop_side"))):
        lo, hi, _ = N.resize_taps(int(bx), int(bw), size, int(side))
        lo2, hi2, _ = N.resize_taps(int(by), int(bh), size, int(side))
        taps = max(taps, int((hi - lo).max() + (hi2 - lo2).max()))
    mean, std, fill = (np.broadcast_to(np.asarray(v, np.float64), (3,)) for v in (mean, std, fill))
    m = np.maximum(1.0, np.abs(fill * std + mean))
    return taps, float(((taps + 12) * U * (m + np.abs(mean)) / std).max())


def windows(params, size):
    """Pixels of the crop that the taps of each 16 x 16 output tile span, per sample: what decides between LDS and L2."""
    out = []
    for bx, by, bw, bh, side in zip(*(params[k] for k in ("box_left", "box_top", "box_w", "box_h", "crop_side"))):
        lx, hx, _ = N.resize_taps(int(bx), int(bw), size, int(side))
        ly, hy, _ = N.resize_taps(int(by), int(bh), size, int(side))
        for t in range(0, size, N.AUG_TILE):
            for s in range(0, size, N.AUG_TILE):
                out.append(int((hx[s:s + N.AUG_TILE].max() - lx[s:s + N.AUG_TILE].min()) * (hy[t:t + N.AUG_TILE].max() - ly[t:t + N.AUG_TILE].min())))
    return np.array(out)


# 96 x 96 -> 128: an upscale, 2 x 2 (at most 3 x 3) taps; 37 x 53 x 1 -> 16: odd, one channel, smaller than a tile; 200 x 150 -> 32: a tent
# of half-width about 4 whose windows fit the LDS; 1024 x 768 -> 16: a window of ~600 x 600, read through L2
@pytest.mark.parametrize("src,size,path", [(0, 128, "lds"), (1, 16, "lds"), (2, 32, "lds"), (3, 16, "l2")])
@pytest.mark.parametrize("bsz", [1, 3])
def test_images_equal_the_definition(pool, src, size, path, bsz):
    from flocoder_amd.augment import augment_images
    ids, idx = ids_for(bsz), np.full(bsz, src)
    params = forced(N.augment_image_params(SEED, ids, pool.hw[idx], size), bsz)
    win = windows(params, size)
    assert (win <= N.AUG_LDS_PIXELS).all() if path == "lds" else (win > N.AUG_LDS_PIXELS).all()
    got = augment_images(pool, idx, ids, size, SEED, params=params)
    ref = N.augment_image_field(SEED, ids, SOURCES, idx, size, params=params)
    assert got.shape == (bsz, 3, size, size) and got.dtype == torch.float32 and got.is_cuda
    taps, bound = image_bound(params, size, 0.5, 0.5, -1.0)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
    print(f"source {src} size {size} B {bsz}: taps {taps} largest error {err:.3e} bound {bound:.3e} fraction {err / bound:.3f}")
    assert err <= bound                                                    # every pixel of every sample


def test_mixed_batch_of_seventy_and_other_statistics(pool):
    """B = 70, the four sources in one batch (LDS and L2 tiles side by side in one launch), drawn angles and flips, then ImageNet's mean and
    std (rounded to fp32 on both sides) with a grey fill."""
    from flocoder_amd.augment import augment_images
    ids, idx = ids_for(70), np.arange(70) % 4
    params = N.augment_image_params(SEED, ids, pool.hw[idx], 32)
    assert params["flip"].any() and not params["flip"].all()
    got = augment_images(pool, idx, ids, 32, SEED).cpu().numpy().astype(np.float64)
    ref = N.augment_image_field(SEED, ids, SOURCES, idx, 32)
    taps, bound = image_bound(params, 32, 0.5, 0.5, -1.0)
    err = np.abs(got - ref).reshape(70, -1).max(axis=1)
    print(f"B 70: taps {taps} largest error {err.max():.3e} bound {bound:.3e} fraction {err.max() / bound:.3f}")
    assert err.max() <= bound
    mean, std = np.float32([0.485, 0.456, 0.406]), np.float32([0.229, 0.224, 0.225])
    fill = np.float32([0.1, -0.2, 0.3])
    got = augment_images(pool, idx[:8], ids[:8], 32, SEED, mean=mean, std=std, fill=fill).cpu().numpy().astype(np.float64)
    ref = N.augment_image_field(SEED, ids[:8], SOURCES, idx[:8], 32, mean=mean.astype(np.float64), std=std.astype(np.float64), fill=fill.astype(np.float64))
    _, bound = image_bound({k: v[:8] for k, v in params.items()}, 32, mean, std, fill)
    assert np.abs(got - ref).max() <= bound


MIDI_SOURCES = [np.random.default_rng(k).integers(0, 256, shape, dtype=np.uint8) * (np.random.default_rng(10 + k).random(shape) < 0.5)
                for k, shape in enumerate([(128, 300, 3), (140, 128, 3), (128, 128, 3), (128, 140, 1), (40, 50, 3)])]
MIDI_SOURCES = [a.astype(np.uint8) for a in MIDI_SOURCES]


@pytest.fixture(scope="module")
def midi_pool():
    from flocoder_amd.augment import ImagePool
    return ImagePool.from_arrays(MIDI_SOURCES, device=DEV)


def midi_params(ids, hw, size, roll):
    p = N.augment_midi_params(SEED, ids, hw, size, roll)
    if roll and ids.size >= 4:                                              # shifts beyond the image, either way and in either axis
        p["roll"][:4] = True
        p["shift_x"][:4] = (int(hw[0][1]), -int(hw[1][1]) - 3, 5, -7)
        p["shift_y"][:4] = (0, 1, int(hw[2][0]) + 2, -24)
    return p


@pytest.mark.parametrize("roll", [True, False])
@pytest.mark.parametrize("gray", [True, False])
@pytest.mark.parametrize("thr", [0.0, 0.3])
@pytest.mark.parametrize("oc", [1, 3])
def test_midi_equals_numpy_in_every_bit(midi_pool, roll, gray, thr, oc):
    from flocoder_amd.augment import augment_midi
    ids, idx = ids_for(70), np.arange(70) % 4                               # 128 x 300, 140 x 128, 128 x 128 (no room to crop), one channel
    p = midi_params(ids, midi_pool.hw[idx], 128, roll)
    got = augment_midi(midi_pool, idx, ids, 128, SEED, roll, gray, thr, oc, params=p)
    ref = N.augment_midi_field(SEED, ids, MIDI_SOURCES, idx, 128, roll, gray, thr, oc, params=p)
    assert got.shape == (70, oc, 128, 128) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy(), ref)
    if roll:
        assert not ref[0].any() and not ref[2].any() and ref[4:].any()
    if thr > 0:
        assert set(np.unique(ref)) == {0.0, 1.0}


@pytest.mark.parametrize("size", [17, 19])
def test_midi_odd_crops_take_the_scalar_stores(midi_pool, size):
    from flocoder_amd.augment import augment_midi
    ids, idx = ids_for(5), np.full(5, 4)
    for gray, thr, oc in ((False, 0.0, 3), (True, 0.3, 1)):
        got = augment_midi(midi_pool, idx, ids, size, SEED, True, gray, thr, oc)
        assert np.array_equal(got.cpu().numpy(), N.augment_midi_field(SEED, ids, MIDI_SOURCES, idx, size, True, gray, thr, oc))
    p = N.augment_midi_params(SEED, ids, midi_pool.hw[idx], size)
    assert len(set(p["crop_left"].tolist())) > 1


def test_rows_streams_and_repeats(pool, midi_pool):
    from flocoder_amd.augment import augment_images, augment_midi
    ids, idx = ids_for(70), np.arange(70) % 3                               # the three sources whose tiles are staged: quick
    whole = augment_images(pool, idx, ids, 32, SEED)
    midi = augment_midi(midi_pool, idx, ids, 128, SEED)
    assert torch.equal(augment_images(pool, idx, ids, 32, SEED), whole) and torch.equal(augment_midi(midi_pool, idx, ids, 128, SEED), midi)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    for k, b in enumerate((0, 13, 37, 69)):
        if k == 2:
            with torch.cuda.stream(side):
                one, m1 = augment_images(pool, idx[b:b + 1], ids[b:b + 1], 32, SEED), augment_midi(midi_pool, idx[b:b + 1], ids[b:b + 1], 128, SEED)
            side.synchronize()
        else:
            one, m1 = augment_images(pool, idx[b:b + 1], ids[b:b + 1], 32, SEED), augment_midi(midi_pool, idx[b:b + 1], ids[b:b + 1], 128, SEED)
        assert torch.equal(one[0], whole[b]) and torch.equal(m1[0], midi[b])
    perm = np.random.default_rng(0).permutation(70)
    assert torch.equal(augment_images(pool, idx[perm], ids[perm], 32, SEED), whole[torch.from_numpy(perm).to(DEV)])
    assert not torch.equal(augment_images(pool, idx, ids, 32, SEED + 1), whole)
    l2 = augment_images(pool, [3, 3], [7, 8], 16, SEED)                     # the path through L2: rows and repeats too
    assert torch.equal(augment_images(pool, [3], [8], 16, SEED)[0], l2[1]) and torch.equal(augment_images(pool, [3, 3], [7, 8], 16, SEED), l2)


def test_abi_errors_launch_nothing(pool):
    from flocoder_amd import _binding as B
    lib = B.lib()
    out = torch.full((2, 3, 16, 16), 7.0, device=DEV)
    stab = torch.from_numpy(N.augment_image_table(N.augment_image_params(SEED, [0, 1], pool.hw[[0, 0]], 16), [0, 0], pool.hw[[0, 0]])).to(DEV)
    mtab = torch.zeros(2, N.AUG_MIDI_WORDS, dtype=torch.int32, device=DEV)
    f3 = lambda *v: (C.c_float * 3)(*v)
    half, zero, bad = f3(0.5, 0.5, 0.5), f3(0.5, 0.0, 0.5), f3(0.5, float("nan"), 0.5)
    stream = B.current_stream(torch.device(DEV))

    def images(out_=out, pool_=pool.buffer, table=pool.table, n=4, stab_=stab, batch=2, size=16, mean=half, std=half, fill=half):
        return lib.fc_augment_images(B.ptr(out_), B.ptr(pool_), B.ptr(table), n, B.ptr(stab_), batch, size, mean, std, fill, stream)

    def midi(out_=out, pool_=pool.buffer, table=pool.table, n=4, stab_=mtab, batch=2, size=16, oc=3, thr=0.3):
        return lib.fc_augment_midi(B.ptr(out_), B.ptr(pool_), B.ptr(table), n, B.ptr(stab_), batch, size, oc, 0, thr, stream)
    errors = (B.FC_E_ARG, B.FC_E_SHAPE)
    for fn in (images, midi):
        for kw in (dict(out_=None), dict(pool_=None), dict(table=None), dict(stab_=None), dict(batch=0), dict(size=8), dict(size=2048), dict(n=0)):
            assert fn(**kw) in errors, (fn.__name__, kw)
    for kw in (dict(std=zero), dict(std=bad), dict(std=f3(0.5, -1.0, 0.5)), dict(mean=None), dict(fill=bad)):
        assert images(**kw) in errors, kw
    assert midi(oc=2) in errors and midi(thr=float("nan")) in errors
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                         # nothing was launched
    assert images() == B.FC_OK and not bool((out == 7.0).any())
    # a source index outside the pool reaches no memory: the sample comes out as the fill (images) or as zero (MIDI)
    stab2 = stab.clone()
    stab2[1, 0] = 99
    assert images(stab_=stab2, fill=f3(0.25, 0.25, 0.25)) == B.FC_OK
    assert torch.allclose(out[1], torch.full_like(out[1], 0.25), rtol=0, atol=1e-6)
    mtab[1, 0] = -3
    assert midi(thr=0.0) == B.FC_OK and not bool(out[1].any())
    from flocoder_amd.augment import augment_images, augment_midi
    for fn in (augment_images, augment_midi):
        with pytest.raises(ValueError):
            fn(pool, [4], [0], 16)
        with pytest.raises(ValueError):
            fn(pool, [0], [0], 8)
    with pytest.raises(ValueError):
        augment_images(pool, [0], [0], 16, std=(0.5, 0.0, 0.5))


def small_vqvae():
    from flocoder_amd.codecs import VQVAE
    g = load_golden("g9_vqvae")
    m = VQVAE(in_channels=1, hidden_channels=32, num_downsamples=4, internal_dim=32, vq_embedding_dim=4).eval()
    m.load_state_dict(synth_state_dict(g["gray_nd4_small_shapes"], 9), strict=False)
    return m.to(DEV)


class RedChannel:
    """The small codec reads one channel: hand it the first of the three."""

    def __init__(self, codec):
        self.codec = codec

    def encode(self, x):
        return self.codec.encode(x[:, :1].contiguous())


def test_end_to_end_preencoding(tmp_path):
    """5 sources x augs_per 4 at batch 8 -> AugmentedBatches -> process_dataset(packed=True) -> PackedLatentDataset: 20 samples, labels
    g % 5, and the stored latents are codec.encode of augment_images / augment_midi of the same ids, batch by batch, bit for bit."""
    from flocoder_amd.augment import AugmentedBatches, ImagePool, augment_images, augment_midi
    from flocoder_amd.data import PackedLatentDataset
    from flocoder_amd.preencode import process_dataset
    codec = small_vqvae()
    srcs = [synthetic(150 + 10 * k, 200 - 10 * k, 3, k) for k in range(5)]
    pool = ImagePool.from_arrays(srcs, labels=[0, 1, 2, 3, 4], device=DEV)
    loader = AugmentedBatches(pool, 4, 8, 128, seed=SEED, first_id=100)
    assert len(loader) == 3
    info = process_dataset(RedChannel(codec), loader, tmp_path / "img", DEV, n_classes=5, packed=True)
    ds = PackedLatentDataset(info["path"])
    assert info["samples"] == 20 and len(ds) == 20
    g = np.arange(20)
    want = torch.cat([RedChannel(codec).encode(augment_images(pool, g[lo:lo + 8] % 5, 100 + g[lo:lo + 8], 128, SEED)) for lo in (0, 8, 16)])
    for i in range(20):
        z, label = ds[i]
        assert int(label) == i % 5 and torch.equal(torch.as_tensor(z).to(DEV), want[i])
    rolls = [a.astype(np.uint8) for a in MIDI_SOURCES[:3]] + [MIDI_SOURCES[0][:, ::-1].copy(), MIDI_SOURCES[1][::-1].copy()]
    mpool = ImagePool.from_arrays(rolls, labels=[0, 1, 2, 3, 4], device=DEV)
    info = process_dataset(codec, AugmentedBatches(mpool, 4, 8, 128, seed=SEED, kind="midi", grayscale=True), tmp_path / "midi", DEV,
                           n_classes=5, packed=True)
    ds = PackedLatentDataset(info["path"])
    want = torch.cat([codec.encode(augment_midi(mpool, g[lo:lo + 8] % 5, g[lo:lo + 8], 128, SEED, grayscale=True)) for lo in (0, 8, 16)])
    assert info["samples"] == 20 and len(ds) == 20 and want.shape == (20, 4, 8, 8)
    for i in range(20):
        z, label = ds[i]
        assert int(label) == i % 5 and torch.equal(torch.as_tensor(z).to(DEV), want[i])
