"""Codebook usage: the counting half of ``flocoder/codebook_analysis.py`` (lines 10-113) on the device.

Which codes of each RVQ level a set of latents uses, and which index combinations, compared between data sets ("val" against "gen" in
``sampling.evaluate_model``).  Upstream builds this from ``bincount`` / ``nonzero`` / a Python loop of ``.item()`` calls and
``torch.unique(...).cpu()`` per update; here ``update_counts`` is one launch of ``fc_index_histogram`` on the indices as
``fc_rvq_quantize`` leaves them -- per-level int64 counts added in place, one int64 key per vector (sum_l idx_l K^l) -- and nothing
waits for the device until somebody reads the statistics.  The plots of the upstream module (matplotlib, plotly, wandb) are not built.
"""
from collections import defaultdict

import torch

from . import _binding as B


class CodebookUsageTracker:
    """codebook_analysis.py:10-61.  ``datasets[name]`` is ``(level_counts, combinations)`` as device tensors: ``level_counts`` int64
    [num_levels, codebook_size], ``combinations`` a pair ``(keys, counts)`` of int64 vectors, the distinct keys in ascending order
    (key = sum_l idx_l * codebook_size**l) and how often each was seen.  ``to_dicts()`` gives upstream's defaultdict form.

    ``update_counts`` queues one kernel and keeps the call's key vector; the distinct keys are merged (``torch.unique`` on the device,
    which sizes its result on the host) when ``datasets`` is next read.  A vector with an index outside [0, codebook_size) is counted at
    no level and in no combination; the number of such vectors is kept on the device and ``check()`` -- called by ``to_dicts``,
    ``calc_usage_stats`` through ``analyze`` -- raises ValueError when it is not zero."""

    def __init__(self, num_levels, codebook_size):
        self.num_levels, self.codebook_size = int(num_levels), int(codebook_size)
        if self.num_levels < 1 or self.codebook_size < 1:
            raise ValueError("CodebookUsageTracker: num_levels and codebook_size must be positive")
        if self.codebook_size ** self.num_levels > 2 ** 63 - 1:
            raise ValueError("CodebookUsageTracker: codebook_size ** num_levels overflows int64, combinations have no key")
        self.reset_all()

    def reset_all(self):
        self._data, self._pending, self._bad = {}, {}, {}

    def reset_dataset(self, name):
        for d in (self._data, self._pending, self._bad):
            d.pop(name, None)

    def add_dataset(self, name, device=None):
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        empty = torch.zeros(0, dtype=torch.int64, device=device)
        self._data[name] = (torch.zeros(self.num_levels, self.codebook_size, dtype=torch.int64, device=device), (empty, empty.clone()))
        self._pending[name] = []
        self._bad[name] = torch.zeros(1, dtype=torch.int64, device=device)

    def update_counts(self, name, indices):
        """indices: device int64 [N, num_levels].  No host synchronisation."""
        if not indices.is_cuda:
            raise RuntimeError("flocoder_amd.CodebookUsageTracker runs on MI355X (gfx950) only; there is no CPU path")
        if indices.dtype != torch.int64 or indices.dim() != 2 or indices.shape[1] != self.num_levels:
            raise ValueError(f"update_counts: indices must be int64 [N, {self.num_levels}], got {indices.dtype} {tuple(indices.shape)}")
        if name not in self._data:
            self.add_dataset(name, indices.device)
        level_counts = self._data[name][0]
        if level_counts.device != indices.device:
            raise ValueError(f"update_counts: data set {name!r} lives on {level_counts.device}, the indices on {indices.device}")
        indices = indices.contiguous()
        keys = torch.empty(indices.shape[0], dtype=torch.int64, device=indices.device)
        with torch.cuda.device(indices.device):
            B.check(B.lib().fc_index_histogram(B.ptr(indices), indices.shape[0], self.num_levels, self.codebook_size, B.ptr(level_counts),
                                               B.ptr(keys), B.ptr(self._bad[name]), B.current_stream(indices.device)))
        self._pending[name].append(keys)

    def _merge(self, name):
        pending = self._pending[name]
        if not pending:
            return
        level_counts, (keys, counts) = self._data[name]
        new = torch.cat(pending)
        k2, c2 = torch.unique(new[new >= 0], return_counts=True)
        uk, inv = torch.unique(torch.cat([keys, k2]), return_inverse=True)
        uc = torch.zeros_like(uk).index_add_(0, inv, torch.cat([counts, c2]))
        self._data[name] = (level_counts, (uk, uc))
        pending.clear()

    @property
    def datasets(self):
        """{name: (level_counts, (keys, counts))} in insertion order, every queued key vector merged."""
        for name in self._data:
            self._merge(name)
        return self._data

    def check(self):
        bad = {name: int(b) for name, b in self._bad.items()}
        bad = {name: b for name, b in bad.items() if b}
        if bad:
            raise ValueError(f"CodebookUsageTracker: vectors with an index outside [0, {self.codebook_size}) were left out: {bad}")

    def to_dicts(self):
        """Upstream's form: {name: ([defaultdict(int) per level: index -> count], defaultdict(int): tuple of indices -> count)}."""
        self.check()
        out = {}
        for name, (level_counts, (keys, counts)) in self.datasets.items():
            lc = level_counts.cpu()
            levels = []
            for l in range(self.num_levels):
                d = defaultdict(int)
                for idx in torch.nonzero(lc[l], as_tuple=True)[0].tolist():
                    d[idx] = int(lc[l, idx])
                levels.append(d)
            combos = defaultdict(int)
            for key, c in zip(keys.tolist(), counts.tolist()):
                combos[tuple((key // self.codebook_size ** l) % self.codebook_size for l in range(self.num_levels))] = c
            out[name] = (levels, combos)
        return out

    def analyze(self, codec, epoch, use_wandb=False, debug=False):
        """codebook_analysis.py:46-61 without the plots: returns ``calc_usage_stats`` of the tracked data sets ({} when there are none)
        and draws nothing.  ``use_wandb=True`` raises: plots and wandb logging are out of scope here."""
        if use_wandb:
            raise NotImplementedError("CodebookUsageTracker.analyze: plots and wandb logging are out of scope; log the returned dictionary")
        if not self._data:
            return {}
        self.check()
        if debug:
            print(f"Running codebook analysis at epoch {epoch}")
        return calc_usage_stats(self.datasets, self.codebook_size)


def _used_sets(entry):
    """(level masks bool [L, K], keys) of one data set, from the tracker's tensors."""
    level_counts, (keys, _) = entry
    return level_counts > 0, keys


def calc_usage_stats(data_dict, codebook_size):
    """codebook_analysis.py:86-113 on the tracker's tensors ({name: (level_counts, (keys, counts))}): the same keys and values --
    ``level_{l}_{name}_usage_pct`` for every data set; with exactly two data sets ``level_{l}_{name2}_only_count`` / ``_only_pct``
    (codes the SECOND name, in insertion order, uses and the first does not; 0 when the second uses none) and ``combo_{name1}_count``,
    ``combo_{name2}_count``, ``combo_{name2}_only_count`` / ``_only_pct``.  Set sizes are formed on the device and cross in one copy; the
    percentages are Python floats as upstream."""
    names = list(data_dict.keys())
    used = {name: _used_sets(data_dict[name]) for name in names}
    num_levels = used[names[0]][0].shape[0]
    cells = [used[name][0].sum(dim=1) for name in names]                       # [L] each
    if len(names) == 2:
        (m1, k1), (m2, k2) = used[names[0]], used[names[1]]
        cells += [(m2 & ~m1).sum(dim=1), (~torch.isin(k2, k1)).sum()]
    flat = torch.cat([c.reshape(-1).long() for c in cells]).tolist()
    per = [flat[i * num_levels:(i + 1) * num_levels] for i in range(len(names))]
    stats = {}
    for level in range(num_levels):
        for i, name in enumerate(names):
            stats[f'level_{level}_{name}_usage_pct'] = per[i][level] / codebook_size * 100
        if len(names) == 2:
            n_only, n2 = flat[2 * num_levels + level], per[1][level]
            stats[f'level_{level}_{names[1]}_only_count'] = n_only
            stats[f'level_{level}_{names[1]}_only_pct'] = n_only / n2 * 100 if n2 else 0
    if len(names) == 2:
        c_only, c1, c2 = flat[3 * num_levels], k1.numel(), k2.numel()
        stats[f'combo_{names[0]}_count'] = c1
        stats[f'combo_{names[1]}_count'] = c2
        stats[f'combo_{names[1]}_only_count'] = c_only
        stats[f'combo_{names[1]}_only_pct'] = c_only / c2 * 100 if c2 else 0
    return stats
