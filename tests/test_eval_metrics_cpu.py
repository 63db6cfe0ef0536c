"""CPU checks of the evaluation metrics' yardsticks and host logic: the restated ``calc_note_metrics`` (tests/note_metrics_ref.py)
against a case counted by hand, the restated ``calc_usage_stats`` (tests/codebook_ref.py) against upstream's formulae on a hand-built
pair of data sets, the package's ``calc_usage_stats`` (plain torch on the tracker's tensors) against the same numbers, and the loud
failures that need no GPU."""
import numpy as np
import pytest
import torch

import codebook_ref as CR
from note_metrics_ref import note_metrics_ref

R, G, K_ = 1.0, 0.5, 0.0                                                 # red (onset), green (sustain), black as grey values
TARGET = [[R, R, G, G],
          [K_, K_, K_, K_],
          [R, G, K_, K_],
          [K_, K_, G, R]]
PRED = [[R, G, G, K_],
        [R, K_, G, K_],
        [R, G, K_, K_],
        [K_, G, G, K_]]
# onset: both red at (0,0) (2,0); pred-only red at (1,0); target-only red at (0,1) (3,3); the other 11 cells are red in neither
# sustain: both green at (0,2) (2,1) (3,2); pred-only green at (0,1) (1,2) (3,1); target-only green at (0,3); the other 9 in neither
HAND = {"onset": (2, 11, 1, 2), "sustain": (3, 9, 3, 1)}


def roll(cells):
    return torch.tensor(cells, dtype=torch.float32).reshape(1, 1, 4, 4)


def test_restated_note_metrics_match_the_hand_count():
    out = note_metrics_ref(roll(PRED), roll(TARGET))
    for i, name in enumerate(("onset", "sustain")):
        tp, tn, fp, fn = HAND[name]
        assert out["counts"][i, 0].tolist() == [tp, tn, fp, fn]
        assert out["metrics"][f"{name}_sensitivity"] == tp / (tp + fn + 1e-8)
        assert out["metrics"][f"{name}_specificity"] == tn / (tn + fp + 1e-8)
        assert out["metrics"][f"{name}_precision"] == tp / (tp + fp + 1e-8)
        assert out["metrics"][f"{name}_f1"] == 2 * tp / (2 * tp + fp + fn + 1e-8)
        for k in ("sensitivity", "specificity", "precision", "f1"):
            assert abs(out["metrics32"][f"{name}_{k}"] - out["metrics"][f"{name}_{k}"]) < 1e-6
        assert out["images"][f"{name}_tp"].shape == (1, 3, 4, 4) and int(out["images"][f"{name}_tp"][0, 0].sum()) == tp
        assert int(out["images"][f"{name}_fn"][0, 2].sum()) == fn
    over = out["images"]["onset_targpred"]                               # target's red cells on red, pred's on green, blue empty
    assert over.shape == (1, 3, 4, 4) and over[0, 2].abs().sum() == 0
    assert torch.equal(over[0, 0], (roll(TARGET)[0, 0] == R).float()) and torch.equal(over[0, 1], (roll(PRED)[0, 0] == R).float())
    # a 3-channel roll of the same cells counts the same (g2rgb passes it through)
    rgb = lambda x: torch.stack([(x[:, 0] == R).float(), (x[:, 0] == G).float(), torch.zeros_like(x[:, 0])], dim=1)
    assert torch.equal(note_metrics_ref(rgb(roll(PRED)), roll(TARGET))["counts"], out["counts"])
    # the region extension: only row 0 counts
    region = torch.zeros(1, 1, 4, 4)
    region[0, 0, 0] = 1.0
    assert note_metrics_ref(roll(PRED), roll(TARGET), region=region)["counts"][:, 0].tolist() == [[1, 2, 0, 1], [1, 1, 1, 1]]


def test_restated_note_metrics_all_black_target_counts_every_pixel_as_true_negative():
    out = note_metrics_ref(roll(PRED), torch.zeros(1, 1, 4, 4))           # min = max = 0: 0 / 0 compares false everywhere
    assert out["counts"][:, 0].tolist() == [[0, 16, 0, 0], [0, 16, 0, 0]]
    assert out["metrics"]["onset_sensitivity"] == 0.0 and out["metrics"]["sustain_f1"] == 0.0
    assert out["metrics"]["onset_specificity"] == 16 / (16 + 1e-8)


VAL = [[0, 1], [0, 1], [1, 2], [3, 0]]
GEN = [[0, 1], [2, 2], [2, 3]]
KSIZE = 4
HAND_STATS = {
    "level_0_val_usage_pct": 75.0, "level_0_gen_usage_pct": 50.0, "level_0_gen_only_count": 1, "level_0_gen_only_pct": 1 / 2 * 100,
    "level_1_val_usage_pct": 75.0, "level_1_gen_usage_pct": 75.0, "level_1_gen_only_count": 1, "level_1_gen_only_pct": 1 / 3 * 100,
    "combo_val_count": 3, "combo_gen_count": 3, "combo_gen_only_count": 2, "combo_gen_only_pct": 2 / 3 * 100,
}


def ref_sets(pairs):
    data = {}
    for name, rows in pairs:
        data[name] = CR.empty_counts(2)
        if rows:
            CR.update_counts(data[name], torch.tensor(rows, dtype=torch.int64))
    return data


def tensor_sets(pairs):
    """The tracker's form of the same data, built by hand on the CPU."""
    data = {}
    for name, rows in pairs:
        idx = torch.tensor(rows, dtype=torch.int64).reshape(-1, 2)
        levels = torch.stack([torch.bincount(idx[:, l], minlength=KSIZE) for l in range(2)])
        keys, counts = torch.unique(idx[:, 0] + KSIZE * idx[:, 1], return_counts=True)
        data[name] = (levels, (keys, counts))
    return data


def test_restated_usage_stats_match_the_hand_count():
    data = ref_sets([("val", VAL), ("gen", GEN)])
    assert dict(data["val"][0][0]) == {0: 2, 1: 1, 3: 1} and dict(data["gen"][1]) == {(0, 1): 1, (2, 2): 1, (2, 3): 1}
    assert CR.calc_usage_stats(data, KSIZE) == HAND_STATS
    keys, counts = CR.keys_of(data["val"][1], KSIZE)
    assert keys.tolist() == [3, 4, 9] and counts.tolist() == [1, 2, 1]
    # an empty second set: the _only_pct branches fall to 0; one set alone: no comparison keys at all
    empty = CR.calc_usage_stats(ref_sets([("val", VAL), ("gen", [])]), KSIZE)
    assert empty["level_0_gen_usage_pct"] == 0 and empty["level_1_gen_only_pct"] == 0 and empty["combo_gen_only_pct"] == 0
    assert empty["combo_gen_count"] == 0 and empty["combo_val_count"] == 3
    assert set(CR.calc_usage_stats(ref_sets([("val", VAL)]), KSIZE)) == {"level_0_val_usage_pct", "level_1_val_usage_pct"}
    # insertion order decides the second name
    assert "combo_val_only_count" in CR.calc_usage_stats(ref_sets([("gen", GEN), ("val", VAL)]), KSIZE)


@pytest.mark.parametrize("pairs", [[("val", VAL), ("gen", GEN)], [("val", VAL), ("gen", [])], [("val", VAL)], [("gen", GEN), ("val", VAL)],
                                   [("a", VAL), ("b", GEN), ("c", VAL)]])
def test_package_usage_stats_equal_the_restatement(pairs):
    from flocoder_amd.codebook_analysis import calc_usage_stats
    got, want = calc_usage_stats(tensor_sets(pairs), KSIZE), CR.calc_usage_stats(ref_sets(pairs), KSIZE)
    assert got == want and list(got) == list(want)
    assert all(type(got[k]) is type(want[k]) for k in want)


def test_new_names_are_exported_and_fail_loudly_without_a_gpu():
    import flocoder_amd as F
    from flocoder_amd import metrics as M
    from flocoder_amd import sampling as S
    assert F.calc_note_metrics is M.calc_note_metrics and F.evaluate_model is S.evaluate_model
    assert F.CodebookUsageTracker(4, 512).datasets == {} and callable(F.calc_usage_stats)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.calc_note_metrics(roll(PRED), roll(TARGET))
    with pytest.raises(RuntimeError, match="no CPU path"):
        F.CodebookUsageTracker(2, 4).update_counts("val", torch.tensor(VAL))
    with pytest.raises(ValueError, match="overflows int64"):
        F.CodebookUsageTracker(8, 512)
    with pytest.raises(NotImplementedError, match="out of scope"):
        F.CodebookUsageTracker(2, 4).analyze(None, 0, use_wandb=True)
    with pytest.raises(NotImplementedError, match="out of scope"):
        S.evaluate_model(None, None, 0, None, use_wandb=True)
    assert F.CodebookUsageTracker(2, 4).analyze(None, 0) == {}
    t, p = roll(TARGET)[0, 0], roll(PRED)[0, 0]
    assert M.targ_pred_mask_to_rgb(t, p).shape == (3, 4, 4) and torch.equal(M.targ_pred_mask_to_rgb(t, p)[1], p)
    assert torch.equal(M.mask_to_rgb(roll(TARGET)[0], color=[1, 0, 2])[:, 2], 2 * roll(TARGET)[0])
