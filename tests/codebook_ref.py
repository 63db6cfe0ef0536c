"""Yardstick for ``flocoder_amd.codebook_analysis``: upstream's counting (flocoder/codebook_analysis.py:28-44) and ``calc_usage_stats``
(86-113) restated on plain Python containers, runnable on the CPU.  A data set is ``(level_counts, combinations)``: one
``{index: count}`` per level and ``{tuple of indices: count}``; a dictionary of data sets keeps insertion order, which decides who is
"name2" in the two-set statistics.  The implementation does not import this file."""
from collections import defaultdict

import numpy as np
import torch


def empty_counts(num_levels):
    return [defaultdict(int) for _ in range(num_levels)], defaultdict(int)


def update_counts(data, indices):
    """Add indices (int64 [N, L], any device) to data = (level_counts, combinations) and return it."""
    level_counts, combinations = data
    idx = indices.cpu()
    for level in range(len(level_counts)):
        counts = torch.bincount(idx[:, level])
        for i in torch.nonzero(counts, as_tuple=True)[0].tolist():
            level_counts[level][i] += int(counts[i])
    combos, combo_counts = torch.unique(idx, dim=0, return_counts=True)
    for combo, count in zip(combos.numpy(), combo_counts.numpy()):
        combinations[tuple(int(c) for c in combo)] += int(count)
    return data


def keys_of(combinations, codebook_size):
    """The package's int64 keys (sum_l idx_l K^l) of upstream's combination tuples, ascending, with their counts."""
    pairs = sorted((sum(int(v) * codebook_size ** l for l, v in enumerate(combo)), c) for combo, c in combinations.items())
    return np.array([k for k, _ in pairs], dtype=np.int64), np.array([c for _, c in pairs], dtype=np.int64)


def calc_usage_stats(data_dict, codebook_size):
    stats = {}
    names = list(data_dict.keys())
    num_levels = len(data_dict[names[0]][0])
    for level in range(num_levels):
        for name, (level_counts, _) in data_dict.items():
            stats[f"level_{level}_{name}_usage_pct"] = len(level_counts[level]) / codebook_size * 100
        if len(names) == 2:
            name1, name2 = names
            set1, set2 = set(data_dict[name1][0][level].keys()), set(data_dict[name2][0][level].keys())
            only = set2 - set1
            stats[f"level_{level}_{name2}_only_count"] = len(only)
            stats[f"level_{level}_{name2}_only_pct"] = len(only) / len(set2) * 100 if set2 else 0
    if len(names) == 2:
        name1, name2 = names
        combos1, combos2 = set(data_dict[name1][1].keys()), set(data_dict[name2][1].keys())
        only = combos2 - combos1
        stats[f"combo_{name1}_count"] = len(combos1)
        stats[f"combo_{name2}_count"] = len(combos2)
        stats[f"combo_{name2}_only_count"] = len(only)
        stats[f"combo_{name2}_only_pct"] = len(only) / len(combos2) * 100 if combos2 else 0
    return stats
