"""Exact k nearest neighbours between latent sets, on the device (csrc/knn.hip; no upstream counterpart).

``d2(a, b) = sum_f (a_f - b_f)^2`` in fp32 by direct differences, one accumulator per pair over the features in ascending order
(``acc = fma(a_f - b_f, a_f - b_f, acc)``), so a copy of a reference comes out at exactly 0 and a pair's d2 has the same bits whichever
of the two is the query and whichever tile, chunk, batch or call it falls in; a non-finite d2 is stored as FLT_MAX.  Neighbours are
ordered by (d2, global reference index): ties go to the lower index and every result is unique.  Samples of any shape are flattened.

- ``knn(queries, refs, k)`` -- ``(d2 [Q,k] fp32, idx [Q,k] int64)``, ascending, missing slots ``(+inf, -1)`` when there are fewer than k
  references;
- ``KnnSearch(queries, k)`` -- the same over references that arrive in chunks (``update`` / ``result``): any split, in any order, gives
  the bits of one call;
- ``nearest_in_dataset(queries, dataset)`` -- over a ``PackedLatentDataset`` walked through its memory map, or any iterable of
  ``(latents, _)`` batches;
- ``ball_counts(queries, refs, radius2)`` -- per query the number of references r with ``d2(q, r) <= radius2[r]``.

``query_ids`` [Q] int64 keeps a point out of its own neighbourhood: the reference whose global index equals ``query_ids[q]`` is skipped
for query q, under chunking as well.  1 <= k <= 64.  Everything runs on the current stream and nothing is read back; CPU tensors raise.

Not built: k > 64, an MFMA GEMM-form prefilter with exact re-check, merging lists across ranks, approximate indices, other metrics such
as cosine."""
import torch

from . import _binding as B

MAX_K = 64


def _rows(x, name):
    if not torch.is_tensor(x):
        raise TypeError(f"flocoder_amd.neighbors: {name} must be a tensor")
    if not x.is_cuda:
        raise RuntimeError(f"flocoder_amd.neighbors runs on MI355X (gfx950) only; there is no CPU path ({name} is a CPU tensor)")
    if x.dim() < 1:
        raise ValueError(f"flocoder_amd.neighbors: {name} must be [rows, ...]")
    return x.reshape(x.shape[0], -1).float().contiguous()


def _ids(query_ids, n, device):
    if query_ids is None:
        return None
    if not torch.is_tensor(query_ids) or query_ids.dtype != torch.int64 or tuple(query_ids.shape) != (n,):
        raise ValueError(f"flocoder_amd.neighbors: query_ids must be an int64 tensor [{n}]")
    if not query_ids.is_cuda:
        raise RuntimeError("flocoder_amd.neighbors runs on MI355X (gfx950) only; there is no CPU path (query_ids is a CPU tensor)")
    return query_ids.to(device).contiguous()


def _check_k(k):
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K:
        raise ValueError(f"flocoder_amd.neighbors: k must be an integer in [1, {MAX_K}], got {k!r}")
    return k


class KnnSearch:
    """The k nearest references of ``queries`` among references that arrive in chunks.  ``update(refs, first_index=None)`` merges the rows
    of ``refs`` as global indices ``first_index .. first_index + len(refs) - 1`` (default: the running count of rows seen so far);
    ``result()`` returns ``(d2 [Q,k], idx [Q,k])``, the running lists themselves, still on the device and not waited for."""

    def __init__(self, queries, k, *, query_ids=None):
        self.k = _check_k(k)
        self.q = _rows(queries, "queries")
        if self.q.shape[0] < 1 or self.q.shape[1] < 1:
            raise ValueError(f"flocoder_amd.neighbors: queries must have at least one row and one feature, got {tuple(self.q.shape)}")
        self.ids = _ids(query_ids, self.q.shape[0], self.q.device)
        self.d2 = torch.full((self.q.shape[0], self.k), float("inf"), dtype=torch.float32, device=self.q.device)
        self.idx = torch.full((self.q.shape[0], self.k), -1, dtype=torch.int64, device=self.q.device)
        self.count = 0

    def update(self, refs, first_index=None):
        r = _rows(refs, "refs")
        if r.device != self.q.device:
            raise ValueError("flocoder_amd.neighbors: queries and refs are on different devices")
        first = self.count if first_index is None else int(first_index)
        if first < 0:
            raise ValueError(f"flocoder_amd.neighbors: first_index must be >= 0, got {first}")
        n = r.shape[0]
        if n and r.shape[1] != self.q.shape[1]:
            raise ValueError(f"flocoder_amd.neighbors: queries have {self.q.shape[1]} features, refs {r.shape[1]}")
        self.count = max(self.count, first + n)
        if n == 0:
            return self
        lib = B.lib()
        nbytes = lib.fc_knn_workspace_bytes(self.q.shape[0], n, self.k)
        if nbytes < 0:
            B.check(int(nbytes))
        dev = self.q.device
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            B.check(lib.fc_knn_update(B.ptr(self.q), self.q.shape[0], B.ptr(r), n, self.q.shape[1], self.k, first, B.ptr(self.ids),
                                      B.ptr(self.d2), B.ptr(self.idx), B.ptr(ws), B.current_stream(dev)))
        return self

    def result(self):
        return self.d2, self.idx


def knn(queries, refs, k, *, query_ids=None):
    """``(d2 [Q,k] fp32, idx [Q,k] int64)``: per query the k nearest rows of ``refs``, ascending in (d2, index)."""
    return KnnSearch(queries, k, query_ids=query_ids).update(refs, 0).result()


def _dataset_chunks(dataset, chunk_rows):
    target = getattr(dataset, "target", None)
    if target is not None and hasattr(dataset, "count"):             # a PackedLatentDataset: rows straight from the memory map, in order
        import numpy as np
        for lo in range(0, dataset.count, chunk_rows):
            yield torch.from_numpy(np.array(target[lo:lo + chunk_rows]))    # a copy: the map is read-only
        return
    for batch in dataset:
        yield batch[0] if isinstance(batch, (tuple, list)) else batch


def nearest_in_dataset(queries, dataset, k=1, chunk_rows=8192):
    """The k nearest items of ``dataset`` for every query: ``(d2, idx)`` with item indices.  ``dataset`` is a ``PackedLatentDataset``,
    read ``chunk_rows`` rows at a time in index order, or any iterable of ``(latents, _)`` batches (indices count its rows in the order
    they arrive).  Chunks go to the queries' device; the run is bound by the host's read and the transfer, not by the kernel."""
    if isinstance(chunk_rows, bool) or not isinstance(chunk_rows, int) or chunk_rows < 1:
        raise ValueError(f"flocoder_amd.neighbors: chunk_rows must be a positive integer, got {chunk_rows!r}")
    search = KnnSearch(queries, k)
    for chunk in _dataset_chunks(dataset, chunk_rows):
        if isinstance(chunk, dict):
            chunk = chunk['target_latents']
        search.update(chunk.to(search.q.device, non_blocking=True))
    return search.result()


def ball_counts(queries, refs, radius2, *, query_ids=None, first_index=0):
    """int32 [Q]: per query the number of rows r of ``refs`` with ``d2(q, r) <= radius2[r]`` (``radius2`` fp32, one per reference; +inf
    counts every reference, NaN none).  ``first_index`` is the global index of ``refs[0]``, which ``query_ids`` refer to."""
    q, r = _rows(queries, "queries"), _rows(refs, "refs")
    if q.shape[0] < 1 or q.shape[1] < 1:
        raise ValueError(f"flocoder_amd.neighbors: queries must have at least one row and one feature, got {tuple(q.shape)}")
    if r.device != q.device:
        raise ValueError("flocoder_amd.neighbors: queries and refs are on different devices")
    n = r.shape[0]
    if n and r.shape[1] != q.shape[1]:
        raise ValueError(f"flocoder_amd.neighbors: queries have {q.shape[1]} features, refs {r.shape[1]}")
    if not torch.is_tensor(radius2) or not radius2.is_cuda or radius2.numel() != n:
        raise ValueError(f"flocoder_amd.neighbors: radius2 must be a device tensor of {n} values, one per reference")
    rad = radius2.reshape(-1).float().contiguous()
    ids = _ids(query_ids, q.shape[0], q.device)
    out = torch.zeros(q.shape[0], dtype=torch.int32, device=q.device)
    if n == 0:
        return out
    with torch.cuda.device(q.device):
        B.check(B.lib().fc_knn_ball_counts(B.ptr(q), q.shape[0], B.ptr(r), n, q.shape[1], B.ptr(rad), int(first_index), B.ptr(ids),
                                           B.ptr(out), B.current_stream(q.device)))
    return out
