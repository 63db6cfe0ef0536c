"""The evaluation metrics on the GPU: ``fc_note_confusion`` through ``metrics.calc_note_metrics`` against the restatement of upstream's
lines (tests/note_metrics_ref.py: counts exactly, images bit for bit, ratios equal to the fp64 formula on those counts and within 1e-6
of upstream's fp32 form -- ratios lie in [0, 1] and that form is three fp32 operations, 3 * 2^-24 = 1.8e-7); ``fc_index_histogram``
through ``CodebookUsageTracker`` against ``torch.bincount`` per level and the restatement's combinations (tests/codebook_ref.py); and
``sampling.evaluate_model`` against its parts composed by hand."""
import numpy as np
import pytest
import torch

import codebook_ref as CR
from conftest import load_golden
from note_metrics_ref import note_metrics_ref
from oracle.synth import synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THR = 0.4
RATIOS = ("sensitivity", "specificity", "precision", "f1")


def boundary_pool(threshold=THR):
    """The values at which g2rgb and the threshold decide, with their fp32 neighbours on both sides, and a few ordinary ones."""
    base = np.array([0.25, 0.5, 0.75, threshold, 1.0], dtype=np.float32)
    near = np.concatenate([base, np.nextafter(base, np.float32(-10)), np.nextafter(base, np.float32(10))])
    return np.concatenate([near, np.array([0.0, -0.3, 0.1, 0.6, 0.9, 1.7], dtype=np.float32)]).astype(np.float32)


def draw(shape, seed, threshold=THR):
    """Half the cells from the boundary pool, half uniform on [-0.2, 1.2]."""
    rng = np.random.default_rng(seed)
    pool = boundary_pool(threshold)
    x = rng.uniform(-0.2, 1.2, size=shape).astype(np.float32)
    pick = rng.random(size=shape) < 0.5
    x[pick] = pool[rng.integers(0, len(pool), size=int(pick.sum()))]
    return torch.from_numpy(x)


def check_against_restatement(pred, target, region=None, **kw):
    from flocoder_amd import metrics as M
    want = note_metrics_ref(pred, target, region=region, **kw)
    metrics, images = M.calc_note_metrics(pred.to(DEV), target.to(DEV), region=None if region is None else region.to(DEV), per_sample=True, **kw)
    counts = metrics["counts"].cpu()
    assert counts.dtype == torch.int64 and torch.equal(counts, want["counts"]), (counts.tolist(), want["counts"].tolist())
    assert set(images) == set(want["images"])
    for k, v in want["images"].items():
        assert images[k].shape == v.shape and torch.equal(images[k].cpu(), v), k
    for k, v in want["metrics"].items():
        assert type(metrics[k]) is float and metrics[k] == v, (k, metrics[k], v)
        assert abs(metrics[k] - want["metrics32"][k]) <= 1e-6, (k, metrics[k], want["metrics32"][k])
    for i, name in enumerate(("onset", "sustain")):
        tp, tn, fp, fn = (want["counts"][i, :, q].double() for q in range(4))
        per = {"sensitivity": tp / (tp + fn + 1e-8), "specificity": tn / (tn + fp + 1e-8), "precision": tp / (tp + fp + 1e-8),
               "f1": 2 * tp / (2 * tp + fp + fn + 1e-8)}
        for k in RATIOS:
            got = metrics["per_sample"][f"{name}_{k}"]
            assert got.dtype == torch.float64 and torch.equal(got.cpu(), per[k]), (name, k)
    none, no_images = M.calc_note_metrics(pred.to(DEV), target.to(DEV), region=None if region is None else region.to(DEV), images=False, **kw)
    assert no_images == {} and none == {k: metrics[k] for k in want["metrics"]}
    return want


# 5x7: odd sizes, one pixel per lane, three samples in one workgroup; 128x128: the workload's image, 16-byte loads, four workgroups per
# sample; 67x63 (4221 pixels, odd) and 72x60 (4320, a multiple of 4): a workgroup's 4096 pixels end inside a sample on either path;
# 130 samples of 5x7: samples that straddle the boundary between two workgroups
@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 128, 128), (2, 67, 63), (3, 72, 60), (130, 5, 7)])
@pytest.mark.parametrize("pc,tc", [(1, 1), (3, 3), (3, 1), (1, 3)])
def test_note_confusion_equals_restatement(shape, pc, tc):
    bsz, h, w = shape
    pred, target = draw((bsz, pc, h, w), 11 * bsz + pc), draw((bsz, tc, h, w), 13 * bsz + tc + 100)
    want = check_against_restatement(pred, target)
    assert int(want["counts"][:, :, [0, 2, 3]].sum()) > 0                # not a trivial all-negative case


@pytest.mark.parametrize("pc,tc", [(1, 1), (3, 1)])
def test_note_confusion_keep_gray_and_explicit_range(pc, tc):
    pred, target = draw((3, pc, 5, 7), 21), draw((3, tc, 5, 7), 22)
    check_against_restatement(pred, target, keep_gray=True)
    pred, target = draw((2, pc, 64, 64), 23), draw((2, tc, 64, 64), 24)
    check_against_restatement(pred, target, keep_gray=True)
    check_against_restatement(pred, target, minval=0.1, maxval=0.9)
    check_against_restatement(pred, target, minval=0.0, maxval=1.0, threshold=0.5)
    check_against_restatement(pred, target, minval=0.25, maxval=0.25)    # a zero range away from zero: +-inf and NaN after the division


def test_note_confusion_all_black_target_and_thresholds():
    pred = draw((3, 1, 5, 7), 31)
    want = check_against_restatement(pred, torch.zeros(3, 1, 5, 7))
    assert want["counts"][:, :, 1].tolist() == [[35] * 3] * 2 and int(want["counts"][:, :, [0, 2, 3]].sum()) == 0
    check_against_restatement(draw((2, 3, 128, 128), 32), torch.zeros(2, 3, 128, 128))
    for thr in (0.25, 0.75):                                             # the pool is rebuilt around the threshold in use
        check_against_restatement(draw((3, 3, 5, 7), 33, thr), draw((3, 1, 5, 7), 34, thr), threshold=thr)


def test_note_confusion_region():
    pred, target = draw((3, 3, 5, 7), 41), draw((3, 1, 5, 7), 42)
    region = draw((3, 1, 5, 7), 43)                                      # 0.5 and its neighbours are among the values
    want = check_against_restatement(pred, target, region=region)
    assert 0 < int(want["counts"][0].sum()) < 3 * 35
    check_against_restatement(pred, target, region=torch.zeros(3, 1, 5, 7))
    pred, target = draw((2, 1, 128, 128), 44), draw((2, 1, 128, 128), 45)
    region = (draw((2, 1, 128, 128), 46) > 0.5).float()
    check_against_restatement(pred, target, region=region)
    want = check_against_restatement(pred, target, region=torch.zeros(2, 1, 128, 128))
    assert int(want["counts"].sum()) == 0


def test_note_confusion_nan_and_inf_in_pred():
    for shape in ((3, 3, 5, 7), (2, 3, 128, 128), (2, 1, 128, 128)):
        pred, target = draw(shape, 51), draw((shape[0], 1) + shape[2:], 52)
        flat = pred.view(-1)
        flat[::7] = float("nan")
        flat[1::11] = float("inf")
        flat[2::13] = float("-inf")
        check_against_restatement(pred, target)
    check_against_restatement(pred, draw((2, 3, 128, 128), 53))          # a derived range that is not [0, 1]


def test_note_confusion_totals_above_2_pow_24_are_exact():
    from flocoder_amd import metrics as M
    red = torch.ones(1, 1, 4096, 4100, device=DEV)
    metrics, images = M.calc_note_metrics(red, red, per_sample=True, images=False)
    assert images == {}
    assert metrics["counts"].cpu().tolist() == [[[16793600, 0, 0, 0]], [[0, 16793600, 0, 0]]]
    assert float(np.float32(16793600 + 1)) != 16793601.0                 # the neighbouring integer is not an fp32
    assert metrics["onset_sensitivity"] == 16793600 / (16793600 + 1e-8) and metrics["sustain_specificity"] == 16793600 / (16793600 + 1e-8)


@pytest.mark.parametrize("hw", [(16, 16), (5, 7)])
def test_note_confusion_misaligned_base_pointer_is_handled(hw):
    """A contiguous tensor whose first element sits 4 bytes past a 16-byte boundary: the call takes the one-pixel-per-lane path."""
    from flocoder_amd import metrics as M
    h, w = hw
    pred, target = draw((2, 3, h, w), 61), draw((2, 1, h, w), 62)
    want = note_metrics_ref(pred, target)

    def shifted(t):
        buf = torch.zeros(t.numel() + 1, device=DEV)
        view = buf.as_strided(tuple(t.shape), tuple(t.stride()), 1)
        view.copy_(t)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        return view

    for p, t in ((shifted(pred), target.to(DEV)), (pred.to(DEV), shifted(target)), (shifted(pred), shifted(target))):
        metrics, images = M.calc_note_metrics(p, t, per_sample=True)
        assert torch.equal(metrics["counts"].cpu(), want["counts"])
        assert all(torch.equal(images[k].cpu(), v) for k, v in want["images"].items())


def test_note_confusion_refuses_what_it_cannot_read():
    from flocoder_amd import metrics as M
    with pytest.raises(ValueError):
        M.calc_note_metrics(torch.zeros(2, 2, 5, 7, device=DEV), torch.zeros(2, 1, 5, 7, device=DEV))
    with pytest.raises(ValueError):
        M.calc_note_metrics(torch.zeros(2, 1, 5, 7, device=DEV), torch.zeros(2, 1, 5, 8, device=DEV))
    with pytest.raises(ValueError):
        M.calc_note_metrics(torch.zeros(2, 1, 5, 7, device=DEV), torch.zeros(2, 1, 5, 7, device=DEV), region=torch.zeros(2, 5, 7, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.calc_note_metrics(torch.zeros(2, 1, 5, 7), torch.zeros(2, 1, 5, 7, device=DEV))


# ---------------------------------------------------------------------------------------------------------------- histogram / tracker
def check_tracker(tracker, name, rows, levels, size):
    """rows: every index row the data set was fed (CPU int64 [N, L])."""
    level_counts, (keys, counts) = tracker.datasets[name]
    assert level_counts.dtype == torch.int64 and level_counts.shape == (levels, size) and level_counts.is_cuda
    for l in range(levels):
        assert torch.equal(level_counts[l].cpu(), torch.bincount(rows[:, l], minlength=size)), l
    ref = CR.update_counts(CR.empty_counts(levels), rows)
    want_keys, want_counts = CR.keys_of(ref[1], size)
    assert np.array_equal(keys.cpu().numpy(), want_keys) and np.array_equal(counts.cpu().numpy(), want_counts)
    got_levels, got_combos = tracker.to_dicts()[name]
    assert [dict(d) for d in got_levels] == [dict(d) for d in ref[0]] and dict(got_combos) == dict(ref[1])
    return ref


@pytest.mark.parametrize("n,levels,size", [(1, 4, 512), (63, 4, 512), (1000, 4, 512), (1000, 1, 3), (300, 2, 37),
                                           (3000, 4, 2048), (3000, 4, 2049)])
def test_histogram_equals_bincount_and_unique(n, levels, size):
    """4 x 2048 = 8192 bins is the largest histogram kept in LDS (FC_HIST_LDS_BINS); 4 x 2049 goes through global atomics."""
    from flocoder_amd import _binding as B
    from flocoder_amd.codebook_analysis import CodebookUsageTracker
    assert B.FC_HIST_LDS_BINS == 8192
    g = torch.Generator().manual_seed(n + levels + size)
    rows = torch.randint(0, size, (n, levels), generator=g)
    rows[: n // 2, 0] = rows[: n // 2, 0] % 5                             # repeated combinations and a crowded corner
    rows[: n // 2, 1:] = rows[: n // 2, 1:] % 2
    rows[-1] = size - 1                                                  # the last bin of every level
    tracker = CodebookUsageTracker(levels, size)
    tracker.update_counts("val", rows.to(DEV))
    check_tracker(tracker, "val", rows, levels, size)


@pytest.mark.parametrize("levels,size", [(4, 512), (4, 2049)])
def test_histogram_all_indices_equal_and_accumulation(levels, size):
    from flocoder_amd.codebook_analysis import CodebookUsageTracker
    tracker = CodebookUsageTracker(levels, size)
    same = torch.full((5000, levels), 7, dtype=torch.int64)              # every lane of every wave on one bin per level
    tracker.update_counts("gen", same.to(DEV))
    level_counts, (keys, counts) = tracker.datasets["gen"]
    assert level_counts[:, 7].tolist() == [5000] * levels and int(level_counts.sum()) == 5000 * levels
    assert keys.tolist() == [sum(7 * size ** l for l in range(levels))] and counts.tolist() == [5000]
    g = torch.Generator().manual_seed(3)
    more = torch.randint(0, 9, (1234, levels), generator=g)
    tracker.update_counts("gen", more.to(DEV))                           # a second call adds to the first
    tracker.update_counts("gen", more[:100].to(DEV))
    check_tracker(tracker, "gen", torch.cat([same, more, more[:100]]), levels, size)
    tracker.reset_dataset("gen")
    assert tracker.datasets == {}


def test_histogram_reports_an_index_out_of_range():
    """Documented behaviour: the row is counted at no level and in no combination, and the tracker raises when its counts are read."""
    from flocoder_amd.codebook_analysis import CodebookUsageTracker
    g = torch.Generator().manual_seed(4)
    rows = torch.randint(0, 16, (500, 3), generator=g)
    bad = rows.clone()
    bad[17, 1], bad[401, 2] = 16, -1
    tracker = CodebookUsageTracker(3, 16)
    tracker.update_counts("val", bad.to(DEV))
    keep = torch.ones(500, dtype=torch.bool)
    keep[[17, 401]] = False
    level_counts, (keys, counts) = tracker.datasets["val"]
    for l in range(3):
        assert torch.equal(level_counts[l].cpu(), torch.bincount(rows[keep][:, l], minlength=16))
    assert int(counts.sum()) == 498 and int(keys.min()) >= 0
    with pytest.raises(ValueError, match="outside"):
        tracker.check()
    with pytest.raises(ValueError, match="outside"):
        tracker.analyze(None, 0)
    with pytest.raises(ValueError):
        tracker.update_counts("val", rows[:, :2].to(DEV))               # the wrong number of levels
    with pytest.raises(ValueError):
        tracker.update_counts("val", rows.to(DEV).int())


# ------------------------------------------------------------------------------------------------------------------- evaluate_model
LEVELS, CODES = 3, 64


def small_models():
    from flocoder_amd.codecs import VQVAE
    from flocoder_amd.unet import Unet
    torch.manual_seed(0)
    model = Unet(dim=8, dim_mults=(1, 2, 4, 8), channels=4, n_classes=10).to(DEV)
    codec = VQVAE(vq_num_embeddings=CODES, codebook_levels=LEVELS, in_channels=1, hidden_channels=32, num_downsamples=4, internal_dim=32,
                  vq_embedding_dim=4).eval()
    codec.load_state_dict(synth_state_dict(load_golden("g9_vqvae")["gray_nd4_small_shapes"], 9), strict=False)
    gen = torch.Generator().manual_seed(1)
    for i in range(LEVELS):                                              # codebooks as tests/test_gpu_vqvae.py initialises them
        codec.vq.layers[i]._codebook.embed.copy_(torch.randn(1, CODES, 4, generator=gen) * (0.5 ** i))
        codec.vq.layers[i]._codebook.initted.fill_(True)
    return model, codec.to(DEV)


def test_evaluate_model_equals_its_parts_composed_by_hand():
    from flocoder_amd import metrics as M
    from flocoder_amd import sampling as S
    from flocoder_amd.codebook_analysis import CodebookUsageTracker
    model, codec = small_models()
    g = torch.Generator().manual_seed(7)
    bsz, steps = 4, 3
    target = torch.randn(6, 4, 8, 8, generator=g).to(DEV)                # more targets than samples: upstream tracks all of them as "val"
    source = torch.randn(bsz, 4, 8, 8, generator=g).to(DEV)
    ids = torch.tensor([0, 3, 9, 5], device=DEV)
    mask = (torch.rand(bsz, 1, 128, 128, generator=g) > 0.6).float().to(DEV)
    kw = dict(method="rk4", batch_size=bsz, n_steps=steps, n_classes=0, latent_shape=(4, 8, 8), cfg_strength=3.0, is_midi=True, keep_gray=False)

    model.eval()
    before = S.sampler(model, codec, cond={"class_cond": ids}, source=source, **kw)
    model.train()
    tracker = CodebookUsageTracker(LEVELS, CODES)
    got, images = S.evaluate_model(model, codec, 5, target, cond={"class_cond": ids}, batch_size=bsz, method="rk4", n_steps=steps, is_midi=True,
                                   cb_tracker=tracker, source=source, mask_pixels=mask, return_images=True)
    assert model.training and not codec.training                        # upstream puts the model back and leaves the codec in eval

    model.eval()
    pred_latents, decoded_pred, nfe = S.sampler(model, codec, cond={"class_cond": ids}, source=source, **kw)
    assert nfe == 4 * steps and torch.equal(pred_latents, before[0]) and torch.equal(decoded_pred, before[1])   # the evaluation left no trace
    decoded_target = S.decode_latents(codec, target[:bsz], True, False)
    assert decoded_pred.shape == (bsz, 3, 128, 128) and decoded_target.shape == (bsz, 3, 128, 128)
    want = M.compute_sample_metrics(pred_latents, target, decoded_pred, decoded_target)
    upstream_keys = {"sinkhorn", "sinkhorn_px", "mse", "mse_px", "pred_mean", "targ_mean", "pred_std", "targ_std", "pred_px_mean", "targ_px_mean",
                     "pred_px_std", "targ_px_std"}
    assert set(want) == upstream_keys
    note = M.calc_note_metrics(decoded_pred, decoded_target, images=False)[0]
    masked = M.calc_note_metrics(decoded_pred, decoded_target, region=mask, images=False)[0]
    want.update({f"note/{k}": v for k, v in note.items()})
    want.update({f"note_masked/{k}": v for k, v in masked.items()})
    print("\n[evaluate_model]", {k: round(v, 6) for k, v in got.items()})
    assert len(note) == 8 and set(got) == set(want)
    for k, v in want.items():
        assert type(got[k]) is float and got[k] == v, (k, got[k], v)     # equal Python floats: every bit
    # the note metrics are those of the restatement on the same images
    ref = note_metrics_ref(decoded_pred.cpu(), decoded_target.cpu())
    assert note == ref["metrics"]
    assert masked == note_metrics_ref(decoded_pred.cpu(), decoded_target.cpu(), region=mask.cpu())["metrics"]

    assert set(images) == {"pred_latents", "target_latents", "decoded_pred", "decoded_target", "source_latents", "decoded_source", "mask_pixels"}
    assert torch.equal(images["pred_latents"], pred_latents) and torch.equal(images["decoded_pred"], decoded_pred)
    assert torch.equal(images["decoded_target"], decoded_target) and torch.equal(images["mask_pixels"], mask)

    # the tracker holds codec.quantize's indices of all targets ("val") and of the generated latents ("gen")
    codec.quantize(target)
    idx_val = codec.indices.cpu()
    codec.quantize(pred_latents)
    idx_gen = codec.indices.cpu()
    assert list(tracker.datasets) == ["val", "gen"]
    ref_sets = {"val": check_tracker(tracker, "val", idx_val, LEVELS, CODES), "gen": check_tracker(tracker, "gen", idx_gen, LEVELS, CODES)}
    stats = tracker.analyze(codec, 5)
    assert stats == CR.calc_usage_stats(ref_sets, CODES) and "combo_gen_only_pct" in stats and "level_2_val_usage_pct" in stats

    # without is_midi / a tracker: upstream's dictionary alone, and the plain return value
    plain = S.evaluate_model(model, codec, 5, target, cond={"class_cond": ids}, batch_size=bsz, n_steps=steps, source=source)
    assert set(plain) == upstream_keys and model.training
    with pytest.raises(NotImplementedError, match="out of scope"):
        S.evaluate_model(model, codec, 5, target, batch_size=bsz, n_steps=steps, source=source, use_wandb=True)
