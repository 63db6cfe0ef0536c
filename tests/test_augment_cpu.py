"""The pre-encoding augmentation's host definitions (``flocoder_amd.noise.augment_*``): the laws of the draws, the geometry against PIL's
own ``rotate`` / ``crop`` / ``resize(box=)`` / ``transpose`` run with the definition's parameters, the MIDI pipeline against
``rotate(0, translate=)`` + ``crop`` exactly, ``BinaryGate`` against torch on every byte, determinism and validation.  No GPU.

No bound here is tuned.  KS: the draws against the law's own n quantile midpoints, a two-sample distance as in the masks' tests, D <=
sqrt(-ln(alpha / 2) / 2) sqrt((n + m) / (n m)) at alpha = 1e-6: 0.060 for n = m = 4000.  Frequencies: |count - n p| <= 5.5 sqrt(n p (1 - p)).
Geometry: 2 grey levels -- PIL rounds to 8 bits after each of its two resize passes (at most 0.5 each) and uses fixed-point
coefficients; a wrong centre or sign moves a checkerboard by whole cells, i.e. by ~255."""
import numpy as np
import pytest

from flocoder_amd import noise as N

SEED, N_IDS = (1 << 32) + 4242, 4000
IDS = np.arange(N_IDS, dtype=np.int64) - 17
Z = 5.5


def ks_bound(n, alpha=1e-6):
    return float(np.sqrt(-np.log(alpha / 2) / 2) * np.sqrt(2.0 / n))


KS_BOUND = ks_bound(N_IDS)


def ks_distance(a, b):
    a, b = np.sort(a), np.sort(b)
    pts = np.concatenate([a, b])
    return float(np.abs(np.searchsorted(a, pts, side="right") / a.size - np.searchsorted(b, pts, side="right") / b.size).max())


def ks_uniform(v, lo, hi):
    """Against the n quantile midpoints of the uniform law on [lo, hi]."""
    v = np.asarray(v, dtype=np.float64)
    return ks_distance(v, lo + (hi - lo) * (np.arange(v.size) + 0.5) / v.size)


def ks_integers(v, lo, hi):
    """Against the n quantile midpoints of the uniform law on the integers lo .. hi."""
    v = np.asarray(v)
    return ks_distance(v, lo + np.floor((np.arange(v.size) + 0.5) / v.size * (hi - lo + 1)))


def freq_ok(count, n, p):
    return abs(count - n * p) <= Z * np.sqrt(n * p * (1 - p))


def synthetic(h, w, channels=3):
    """A gradient plus a one-pixel checkerboard: a shift by one pixel in either axis changes a channel by 255."""
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([x * 255 // (w - 1), y * 255 // (h - 1), ((x + y) % 2) * 255], axis=-1).astype(np.uint8)
    return a if channels == 3 else (a[:, :, 2:3] // 2 + a[:, :, 0:1] // 2).astype(np.uint8)


@pytest.fixture(scope="module")
def image_params():
    return N.augment_image_params(SEED, IDS, (375, 500), 128)


def test_ks_bound_is_the_stated_one():
    assert abs(KS_BOUND - 0.060) < 5e-4


def test_image_parameter_laws(image_params):
    p = image_params
    d = ks_uniform(p["angle"], -15.0, 15.0)
    print("angle KS", d, "bound", KS_BOUND)
    assert d <= KS_BOUND and p["angle"].min() >= -15.0 and p["angle"].max() <= 15.0
    side = int(0.9 * 375)
    assert (p["crop_side"] == side).all() and (p["crop_top"] == round((375 - side) / 2.0)).all() and (p["crop_left"] == round((500 - side) / 2.0)).all()
    hit = p["tries"] < N.AUG_TRIES
    assert (p["area_frac"][hit] >= 0.8).all() and (p["area_frac"][hit] <= 1.0).all()
    assert (p["ratio"][hit] >= 3 / 4).all() and (p["ratio"][hit] <= 4 / 3).all()
    assert np.array_equal(p["box_w"][hit], np.rint(np.sqrt(side * side * p["area_frac"][hit] * p["ratio"][hit])))
    assert np.array_equal(p["box_h"][hit], np.rint(np.sqrt(side * side * p["area_frac"][hit] / p["ratio"][hit])))
    assert (p["box_w"] >= 1).all() and (p["box_left"] >= 0).all() and (p["box_left"] + p["box_w"] <= side).all()
    assert (p["box_h"] >= 1).all() and (p["box_top"] >= 0).all() and (p["box_top"] + p["box_h"] <= side).all()
    assert freq_ok(int(p["flip"].sum()), N_IDS, 0.5)
    # the offsets are uniform over the positions that fit: offset / (positions) is uniform on [0, 1) up to the integer step
    room = hit & (side - p["box_w"] >= 20)
    u = (p["box_left"][room] + 0.5) / (side - p["box_w"][room] + 1)
    bound = ks_bound(int(room.sum())) + 0.5 / 21
    print("box_left KS", ks_uniform(u, 0.0, 1.0), "bound", bound)
    assert ks_uniform(u, 0.0, 1.0) <= bound


def test_fallback_box(image_params):
    """A try is rejected where w or h exceeds the crop's side: at side 337 that is |ln ratio| > -ln(area fraction), probability 0.626 a
    try (1 - (0.2 - 0.8 ln 1.25) / (0.2 ln(4/3))), so ten in a row 0.0092 a sample: 37 of 4000, held within z = 5.5.  The fallback of
    a square is the whole crop.  On a 10 x 400 source the centre crop is 9 x 9 -- square again, whatever the source's ratio -- and
    rounding lets w = 9 stand for sqrt(area ratio) up to 9.5, so a rejection is rare there and ten in a row are not seen; its boxes
    all fit."""
    p = image_params
    fb = p["tries"] == N.AUG_TRIES
    q = (1 - (0.2 - 0.8 * np.log(1.25)) / (0.2 * np.log(4 / 3))) ** 10
    print("fallbacks", int(fb.sum()), "of", N_IDS, "expected", N_IDS * q)
    assert freq_ok(int(fb.sum()), N_IDS, q) and fb.any()
    side = int(0.9 * 375)
    assert (p["box_w"][fb] == side).all() and (p["box_h"][fb] == side).all() and (p["box_top"][fb] == 0).all() and (p["box_left"][fb] == 0).all()
    assert np.isnan(p["ratio"][fb]).all() and not np.isnan(p["ratio"][~fb]).any()
    thin = N.augment_image_params(SEED, IDS, (10, 400), 16)
    assert (thin["crop_side"] == 9).all() and (thin["crop_top"] == 0).all() and (thin["crop_left"] == 196).all()
    assert (thin["box_w"] <= 9).all() and (thin["box_h"] <= 9).all() and (thin["box_left"] + thin["box_w"] <= 9).all()
    whole = thin["tries"] == N.AUG_TRIES
    assert (thin["box_w"][whole] == 9).all() and (thin["box_h"][whole] == 9).all()
    a = N.augment_image_field(SEED, IDS[:8], [synthetic(10, 400)], np.zeros(8, int), 16)
    assert np.isfinite(a).all() and np.abs(a).max() <= 1.0


def test_midi_parameter_laws():
    p = N.augment_midi_params(SEED, IDS, (128, 512), 128)
    assert freq_ok(int(p["roll"].sum()), N_IDS, 0.5)
    r = p["roll"]
    bound = ks_bound(int(r.sum()))
    assert p["shift_x"][r].min() >= -256 and p["shift_x"][r].max() <= 256 and p["shift_y"][r].min() >= -24 and p["shift_y"][r].max() <= 24
    assert ks_integers(p["shift_x"][r], -256, 256) <= bound and ks_integers(p["shift_y"][r], -24, 24) <= bound
    assert (p["shift_x"][~r] == 0).all() and (p["shift_y"][~r] == 0).all()
    assert (p["crop_top"] == 0).all() and ks_integers(p["crop_left"], 0, 384) <= KS_BOUND
    off = N.augment_midi_params(SEED, IDS, (128, 512), 128, random_roll=False)
    assert not off["roll"].any() and (off["shift_x"] == 0).all() and np.array_equal(off["crop_left"], p["crop_left"])
    with pytest.raises(ValueError):
        N.augment_midi_params(SEED, IDS[:2], (100, 512), 128)


def pil_image_pipeline(Image, a, p, b, size, fill_byte=0):
    im = Image.fromarray(a if a.shape[2] == 3 else a[:, :, 0])
    fillcolor = fill_byte if a.shape[2] == 1 else (fill_byte,) * 3
    r = im.rotate(float(p["angle"][b]), Image.NEAREST, fillcolor=fillcolor)
    t, l, s = int(p["crop_top"][b]), int(p["crop_left"][b]), int(p["crop_side"][b])
    c = r.crop((l, t, l + s, t + s))
    bx, by, bw, bh = (int(p[k][b]) for k in ("box_left", "box_top", "box_w", "box_h"))
    o = c.resize((size, size), Image.BILINEAR, box=(bx, by, bx + bw, by + bh))
    if p["flip"][b]:
        o = o.transpose(Image.FLIP_LEFT_RIGHT)
    o = np.asarray(o, dtype=np.float64)
    return (o[:, :, None].repeat(3, axis=2) if o.ndim == 2 else o).transpose(2, 0, 1)


@pytest.mark.parametrize("hw,channels,size", [((150, 200), 3, 32), ((150, 200), 3, 128), ((53, 37), 3, 16), ((53, 37), 1, 16)])
def test_image_geometry_against_pil(hw, channels, size):
    Image = pytest.importorskip("PIL.Image")
    a = synthetic(*hw, channels)
    ids = IDS[:24]
    p = N.augment_image_params(SEED, ids, hw, size)
    p["angle"][:3] = (-15.0, 0.0, 15.0)
    p["flip"][:4] = (True, False, True, False)
    field = N.augment_image_field(SEED, ids, [a], np.zeros(ids.size, int), size, params=p)
    assert field.shape == (ids.size, 3, size, size) and field.dtype == np.float64
    worst = 0.0
    for b in range(ids.size):
        worst = max(worst, float(np.abs((field[b] * 0.5 + 0.5) * 255.0 - pil_image_pipeline(Image, a, p, b, size)).max()))
    print(hw, channels, size, "largest difference to PIL, grey levels:", worst)
    assert worst <= 2.0
    # fill: a grey fill of byte 128 in output units, against PIL's fillcolor=128
    grey = N.augment_image_field(SEED, ids[:3], [a], np.zeros(3, int), size, fill=128 / 255 * 2 - 1, params={k: v[:3] for k, v in p.items()})
    for b in range(3):
        assert np.abs((grey[b] * 0.5 + 0.5) * 255.0 - pil_image_pipeline(Image, a, p, b, size, 128)).max() <= 2.0


def test_image_normalisation_and_channels():
    a = synthetic(53, 37, 1)
    ids = IDS[:4]
    one = N.augment_image_field(SEED, ids, [a], np.zeros(4, int), 16)
    three = N.augment_image_field(SEED, ids, [np.repeat(a, 3, axis=2)], np.zeros(4, int), 16)
    assert np.array_equal(one, three) and np.array_equal(one[:, 0], one[:, 2])
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    other = N.augment_image_field(SEED, ids, [a], np.zeros(4, int), 16, mean=mean, std=std, fill=(-np.array(mean) / np.array(std)))
    for c in range(3):
        assert np.allclose(other[:, c] * std[c] + mean[c], one[:, c] * 0.5 + 0.5, rtol=0, atol=1e-12)


def pil_midi(Image, a, p, b, size):
    im = Image.fromarray(a if a.shape[2] == 3 else a[:, :, 0])
    if p["roll"][b]:
        im = im.rotate(0, translate=(int(p["shift_x"][b]), int(p["shift_y"][b])))
    t, l = int(p["crop_top"][b]), int(p["crop_left"][b])
    o = np.asarray(im.crop((l, t, l + size, t + size)))
    return (o[:, :, None] if o.ndim == 2 else o).transpose(2, 0, 1)


@pytest.mark.parametrize("hw,channels", [((128, 300), 3), ((140, 128), 3), ((128, 128), 1)])
def test_midi_against_pil(hw, channels):
    """rotate(0, translate=(h, v)) then crop equals the definition exactly: positive shifts move the image right and down, zero fill."""
    Image = pytest.importorskip("PIL.Image")
    a = np.random.default_rng(5).integers(0, 256, (*hw, channels), dtype=np.uint8)
    ids = IDS[:40]
    p = N.augment_midi_params(SEED, ids, hw, 128)
    p["roll"][:4] = True
    p["shift_x"][:4] = (hw[1], -hw[1] - 3, 5, -7)                       # the whole image pushed out, either way
    p["shift_y"][:4] = (0, 0, 200, -24)
    assert p["roll"].any() and not p["roll"].all()
    got = N.augment_midi_field(SEED, ids, [a], np.zeros(ids.size, int), 128, binary_thresh=0.0, params=p)
    assert got.dtype == np.float32 and got.shape == (ids.size, 3, 128, 128)
    for b in range(ids.size):
        want = np.broadcast_to(pil_midi(Image, a, p, b, 128), (3, 128, 128)).astype(np.float32) / np.float32(255.0)
        assert np.array_equal(got[b], want), b
    assert not got[0].any() and not got[1].any() and not got[2].any()


def test_midi_gray_gate_and_channels():
    a = np.random.default_rng(6).integers(0, 256, (128, 300, 3), dtype=np.uint8)
    ids, src = IDS[:6], np.zeros(6, int)
    raw = N.augment_midi_field(SEED, ids, [a], src, 128, binary_thresh=0.0)
    gray = N.augment_midi_field(SEED, ids, [a], src, 128, grayscale=True, binary_thresh=0.0)
    assert gray.shape == (6, 1, 128, 128)
    assert np.array_equal(gray[:, 0], np.clip((raw[:, 0] + raw[:, 1]) + raw[:, 2], np.float32(0), np.float32(1))) and gray.max() == 1.0
    gated = N.augment_midi_field(SEED, ids, [a], src, 128)
    assert np.array_equal(gated, (raw >= np.float32(0.3)).astype(np.float32))
    g3 = N.augment_midi_field(SEED, ids, [a], src, 128, grayscale=True, out_channels=3)
    assert g3.shape == (6, 3, 128, 128) and np.array_equal(g3[:, 2], (gray[:, 0] >= np.float32(0.3)).astype(np.float32))
    first = N.augment_midi_field(SEED, ids, [a], src, 128, out_channels=1)
    assert np.array_equal(first[:, 0], gated[:, 0])


def test_binary_gate_equals_torch_on_every_byte():
    """All 256 bytes through ToTensor's /255 and BinaryGate(0.3) in torch fp32 on the CPU; 76 / 255 = 0.298 and 77 / 255 = 0.302 straddle it."""
    import torch
    a = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)
    p = {"roll": np.zeros(1, bool), "shift_x": np.zeros(1, int), "shift_y": np.zeros(1, int), "crop_top": np.zeros(1, int), "crop_left": np.zeros(1, int)}
    for thr in (0.3, 0.5, 76 / 255, 1.0):
        got = N.augment_midi_field(0, [0], [a], [0], 16, binary_thresh=thr, out_channels=1, params=p)[0, 0].reshape(-1)
        t = torch.from_numpy(a.reshape(-1).copy()).to(torch.float32).div(255)
        want = torch.where(t >= thr, torch.ones_like(t), torch.zeros_like(t)).numpy()
        assert np.array_equal(got, want), thr
    got = N.augment_midi_field(0, [0], [a], [0], 16, out_channels=1, params=p)[0, 0].reshape(-1)
    assert got[76] == 0.0 and got[77] == 1.0
    plain = N.augment_midi_field(0, [0], [a], [0], 16, binary_thresh=0.0, out_channels=1, params=p)[0, 0].reshape(-1)
    assert np.array_equal(plain, torch.arange(256, dtype=torch.float32).div(255).numpy())


def test_same_seed_and_id_same_bits_whatever_the_batch():
    srcs = [synthetic(53, 37), synthetic(60, 44, 1)]
    ids = np.array([-5, 3, (1 << 32) + 9, 11], dtype=np.int64)
    src = np.array([0, 1, 1, 0])
    whole = N.augment_image_field(SEED, ids, srcs, src, 16)
    midi_srcs = [np.random.default_rng(k).integers(0, 256, (40, 50, 3), dtype=np.uint8) for k in range(2)]
    midi = N.augment_midi_field(SEED, ids, midi_srcs, src, 32)
    for b in (0, 2, 3):
        assert np.array_equal(N.augment_image_field(SEED, ids[b:b + 1], srcs, src[b:b + 1], 16)[0], whole[b])
        assert np.array_equal(N.augment_midi_field(SEED, ids[b:b + 1], midi_srcs, src[b:b + 1], 32)[0], midi[b])
    perm = np.array([2, 0, 3, 1])
    assert np.array_equal(N.augment_image_field(SEED, ids[perm], srcs, src[perm], 16), whole[perm])
    assert not np.array_equal(N.augment_image_field(SEED + 1, ids, srcs, src, 16), whole)
    t = N.augment_image_table(N.augment_image_params(SEED, ids, [(53, 37), (60, 44), (60, 44), (53, 37)], 16), src, [(53, 37), (60, 44), (60, 44), (53, 37)])
    assert t.dtype == np.int32 and t.shape == (4, N.AUG_IMAGE_WORDS)


def test_key_offset_differs_from_the_other_fields():
    assert len({N.AUG_KEY_OFFSET, N.MASK_KEY_OFFSET, N.PROBE_KEY_OFFSET, 0}) == 4
    ids = np.arange(8)
    aug = N.aug_words(SEED, ids, 0, 0)
    assert not np.array_equal(aug, N.mask_words(SEED, ids, 0, 0))
    assert not np.array_equal(aug[:, :].astype(np.uint32), N.field_words(SEED, 0, ids, 4)[:, 0])
    assert not np.array_equal(aug[:, :].astype(np.uint32), N.field_words((SEED + N.PROBE_KEY_OFFSET) & 0xffffffffffffffff, 0, ids, 4)[:, 0])
    assert np.array_equal(N.aug_words(SEED, ids, 0, 0), N.mask_words(SEED + N.AUG_KEY_OFFSET - N.MASK_KEY_OFFSET, ids, 0, 0))


def test_validation():
    from flocoder_amd.augment import AugmentedBatches, ImagePool, augment_images, augment_midi
    srcs = [synthetic(53, 37), synthetic(60, 44)]
    with pytest.raises(ValueError):
        N.augment_image_field(SEED, [0], srcs, [2], 16)
    with pytest.raises(ValueError):
        N.augment_midi_field(SEED, [0], srcs, [-1], 16)
    for size in (8, 2048):
        with pytest.raises(ValueError):
            N.augment_image_params(SEED, [0], (53, 37), size)
    with pytest.raises(ValueError):
        ImagePool.from_arrays(srcs, labels=[0], device="cpu")
    with pytest.raises(ValueError):
        ImagePool.from_arrays([srcs[0].astype(np.float32)], device="cpu")
    pool = ImagePool.from_arrays(srcs, labels=[3, 4], device="cpu")
    assert len(pool) == 2 and pool.nbytes >= sum(a.size for a in srcs) and pool.labels.tolist() == [3, 4]
    for fn in (augment_images, augment_midi):
        with pytest.raises(ValueError):
            fn(pool, [2], [0], 16)
        with pytest.raises(ValueError):
            fn(pool, [0, 1], [0], 16)
        with pytest.raises(RuntimeError):
            fn(pool, [1], [0], 16)                                     # a pool on the CPU: there is no CPU path
    with pytest.raises(RuntimeError):
        AugmentedBatches(pool, 2, 4, 16)


def test_pool_from_files(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from flocoder_amd.augment import ImagePool
    srcs = [synthetic(20, 30), synthetic(24, 18, 1)]
    paths = []
    for k, a in enumerate(srcs):
        paths.append(str(tmp_path / f"{k}.png"))
        Image.fromarray(a if a.shape[2] == 3 else a[:, :, 0]).save(paths[-1])
    pool = ImagePool.from_files(paths, labels=[1, 0], device="cpu")
    assert len(pool) == 2 and pool.hw.tolist() == [[20, 30], [24, 18]] and pool.channels.tolist() == [3, 1]
    assert all(np.array_equal(a, b) for a, b in zip(pool.arrays, srcs))
    rgb = ImagePool.from_files(paths, device="cpu", mode="RGB")
    assert rgb.channels.tolist() == [3, 3] and rgb.labels.tolist() == [0, 0]
