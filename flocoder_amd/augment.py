"""Pre-encoding augmentation on the device (csrc/augment.hip): upstream's ``image_transforms`` and ``midi_transforms``
(flocoder/data.py:49-111) from a pool of decoded source images that stays resident on the GPU as uint8.

Every source is decoded once (``ImagePool``); an augmented batch is then one launch (``augment_images`` / ``augment_midi``) that writes the
fp32 NCHW tensor ``codec.encode`` reads, and ``AugmentedBatches`` walks ``len(pool) * augs_per`` items in the batches
``preencode.process_dataset`` consumes.  The output is defined by ``flocoder_amd.noise.augment_image_field`` / ``augment_midi_field``
(NumPy); the draws are counter-based -- a variant is a function of (seed, sample id, source) and of nothing else -- and are made on the
host, a row of integers per sample, so the device only reads a small table.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _binding as B
from . import noise as N

_NO_CPU = "flocoder_amd.{} runs on MI355X (gfx950) only; there is no CPU path (flocoder_amd.noise.{} is the NumPy form)"
IMAGE_MEAN = IMAGE_STD = (0.5, 0.5, 0.5)


class ImagePool:
    """Decoded source images, resident as ONE uint8 buffer of HWC images on ``device`` plus the int64 table ``(byte offset, H, W, C)`` the
    kernels read.  ``labels``: one class per source (default 0).  A pool on the CPU can be built (``hw``, ``labels`` and the arrays, for
    the NumPy forms) but not augmented from."""

    def __init__(self, arrays, labels=None, device="cuda"):
        arrays = [N._source_bytes(a) for a in arrays]
        if not arrays:
            raise ValueError("ImagePool: no source")
        if labels is None:
            labels = [0] * len(arrays)
        labels = [int(v) for v in labels]
        if len(labels) != len(arrays):
            raise ValueError(f"ImagePool: {len(labels)} labels for {len(arrays)} sources")
        for a in arrays:
            if min(a.shape[:2]) < 2 or max(a.shape[:2]) > N.AUG_MAX_SIDE:
                raise ValueError(f"ImagePool: a source of {a.shape[0]} x {a.shape[1]}: sides must lie in [2, {N.AUG_MAX_SIDE}]")
        self.device = torch.device(device)
        self.labels = torch.tensor(labels, dtype=torch.long)
        self.hw = np.array([a.shape[:2] for a in arrays], dtype=np.int64)
        self.channels = np.array([a.shape[2] for a in arrays], dtype=np.int64)
        sizes = np.array([a.size for a in arrays], dtype=np.int64)
        padded = (sizes + 15) // 16 * 16                                  # every source starts on a 16-byte boundary
        self.offsets = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
        self.nbytes = int(padded.sum())
        self.arrays = arrays if self.device.type != "cuda" else None
        self.buffer = self.table = None
        if self.device.type == "cuda":
            self.buffer = torch.zeros(self.nbytes, dtype=torch.uint8, device=self.device)
            for a, off in zip(arrays, self.offsets):
                self.buffer[int(off):int(off) + a.size].copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
            table = np.stack([self.offsets, self.hw[:, 0], self.hw[:, 1], self.channels], axis=1)
            self.table = torch.from_numpy(np.ascontiguousarray(table)).to(self.device)

    @classmethod
    def from_arrays(cls, arrays, labels=None, device="cuda"):
        """``arrays``: uint8 ``[H, W, 3]``, ``[H, W, 1]`` or ``[H, W]`` each."""
        return cls(arrays, labels, device)

    @classmethod
    def from_files(cls, paths, labels=None, device="cuda", mode=None):
        """Decodes each file once with PIL.  ``mode``: "RGB" or "L" converts every file; by default a file that is neither is converted
        to RGB."""
        try:
            from PIL import Image
        except ImportError as e:
            raise RuntimeError("ImagePool.from_files needs PIL (Pillow) to decode image files; it is not installed -- decode the files "
                               "yourself and use ImagePool.from_arrays") from e
        arrays = []
        for p in paths:
            with Image.open(p) as im:
                if mode is not None:
                    im = im.convert(mode)
                elif im.mode not in ("RGB", "L"):
                    im = im.convert("RGB")
                arrays.append(np.asarray(im, dtype=np.uint8).copy())
        return cls(arrays, labels, device)

    def __len__(self):
        return len(self.hw)


def _tables(pool, src_index, sample_ids, what):
    src = np.asarray(torch.as_tensor(src_index).cpu(), dtype=np.int64).reshape(-1)
    ids = np.asarray(torch.as_tensor(sample_ids).cpu(), dtype=np.int64).reshape(-1)
    if src.size != ids.size or src.size < 1:
        raise ValueError(f"{what}: {src.size} source indices for {ids.size} sample ids (at least one of each)")
    if src.min() < 0 or src.max() >= len(pool):
        raise ValueError(f"{what}: source index outside [0, {len(pool)})")
    return src, ids


def _require_device(pool, what, form):
    if pool.device.type != "cuda":
        raise RuntimeError(_NO_CPU.format(what, form))


def _image_host(pool, src_index, sample_ids, image_size, seed, params=None):
    """The host half of ``augment_images``: validation and the sample table (NumPy only, so it can run beside the GPU's work)."""
    src, ids = _tables(pool, src_index, sample_ids, "augment_images")
    s = N._check_aug_size(image_size)
    hw = pool.hw[src]
    if params is None:
        params = N.augment_image_params(seed, ids, hw, s)
    return ids.size, s, N.augment_image_table(params, src, hw)


def _image_launch(pool, job, mean=IMAGE_MEAN, std=IMAGE_STD, fill=-1.0):
    n, s, table = job
    vals = [np.broadcast_to(np.asarray(v, dtype=np.float32), (3,)) for v in (mean, std, fill)]
    if not all(np.isfinite(v).all() for v in vals) or not (vals[1] > 0).all():
        raise ValueError("augment_images: mean, std and fill must be finite and std positive")
    _require_device(pool, "augment_images", "augment_image_field")
    m, sd, fl = ((ctypes.c_float * 3)(*[float(x) for x in v]) for v in vals)
    stab = torch.from_numpy(table).to(pool.device)
    out = torch.empty(n, 3, s, s, dtype=torch.float32, device=pool.device)
    B.check(B.lib().fc_augment_images(B.ptr(out), B.ptr(pool.buffer), B.ptr(pool.table), len(pool), B.ptr(stab), n, s, m, sd, fl,
                                      B.current_stream(pool.device)))
    return out


def augment_images(pool, src_index, sample_ids, image_size=128, seed=0, mean=IMAGE_MEAN, std=IMAGE_STD, fill=-1.0, params=None):
    """fp32 ``[B, 3, S, S]`` on the pool's device: row b is upstream's ``image_transforms(image_size)`` of source ``src_index[b]`` under
    the draws of ``(seed, sample_ids[b])`` -- rotation by up to 15 degrees, centre crop to 90 %, ``RandomResizedCrop(scale=(0.8, 1))``
    with PIL's antialiased bilinear resize, horizontal flip, ``Normalize(mean, std)`` -- as ``noise.augment_image_field`` defines it.
    ``fill`` (output units; a scalar or three values) is what lies outside the rotated source: -1.0, black, by default (see the
    definition's note on upstream's ``fill``).  ``params``: ``noise.augment_image_params``' dict with entries replaced."""
    return _image_launch(pool, _image_host(pool, src_index, sample_ids, image_size, seed, params), mean, std, fill)


def _midi_host(pool, src_index, sample_ids, image_size, seed, random_roll=True, params=None):
    src, ids = _tables(pool, src_index, sample_ids, "augment_midi")
    s = N._check_aug_size(image_size)
    if params is None:
        params = N.augment_midi_params(seed, ids, pool.hw[src], s, random_roll)
    return ids.size, s, N.augment_midi_table(params, src)


def _midi_launch(pool, job, grayscale=False, binary_thresh=0.3, out_channels=None):
    n, s, table = job
    oc = int(out_channels) if out_channels is not None else (1 if grayscale else 3)
    if oc not in (1, 3):
        raise ValueError("augment_midi: out_channels is 1 or 3")
    _require_device(pool, "augment_midi", "augment_midi_field")
    stab = torch.from_numpy(table).to(pool.device)
    out = torch.empty(n, oc, s, s, dtype=torch.float32, device=pool.device)
    B.check(B.lib().fc_augment_midi(B.ptr(out), B.ptr(pool.buffer), B.ptr(pool.table), len(pool), B.ptr(stab), n, s, oc,
                                    1 if grayscale else 0, float(binary_thresh), B.current_stream(pool.device)))
    return out


def augment_midi(pool, src_index, sample_ids, image_size=128, seed=0, random_roll=True, grayscale=False, binary_thresh=0.3,
                 out_channels=None, params=None):
    """fp32 ``[B, out_channels, S, S]`` on the pool's device: upstream's ``midi_transforms`` -- ``RandomRoll`` (a translation with zero
    fill, p = 0.5), ``RandomCrop(image_size)``, ``ToTensor``, optionally ``MyRGBToGrayscale`` and, for ``binary_thresh > 0``,
    ``BinaryGate`` -- equal to ``noise.augment_midi_field`` in every bit.  ``out_channels``: 1 or 3, default 1 with ``grayscale`` else 3."""
    if out_channels is not None and int(out_channels) not in (1, 3):
        raise ValueError("augment_midi: out_channels is 1 or 3")
    return _midi_launch(pool, _midi_host(pool, src_index, sample_ids, image_size, seed, random_roll, params), grayscale, binary_thresh, out_channels)


class AugmentedBatches:
    """The pre-encoding loader: ``len(pool) * augs_per`` augmented items in batches of ``batch_size``, each ``(images on the device,
    classes)`` -- what ``preencode.process_dataset`` consumes unchanged.  Item g is source ``g % len(pool)`` under sample id
    ``first_id + g``, so a run is a function of (seed, first_id) whatever the batch size.  ``kind``: "image" (``augment_images``) or
    "midi" (``augment_midi``); ``transform_kwargs`` go to that function.  The host half of a batch -- the draws and the sample table,
    NumPy -- is made one batch ahead on a worker thread, beside the encode of the batch before; the launch stays on the caller's thread
    and stream.

    ``process_dataset(rank=, world=)`` skips the batches of other ranks AFTER they have been generated; a generated batch is one launch,
    cheap next to the encode it precedes, so every rank simply walks the same iterator."""

    def __init__(self, pool, augs_per, batch_size, image_size, seed=0, kind="image", first_id=0, **transform_kwargs):
        if kind not in ("image", "midi"):
            raise ValueError(f"kind={kind!r}: 'image' or 'midi'")
        if int(augs_per) < 1 or int(batch_size) < 1:
            raise ValueError("augs_per and batch_size must be positive")
        if pool.device.type != "cuda":
            raise RuntimeError(_NO_CPU.format("AugmentedBatches", "augment_image_field / augment_midi_field"))
        allowed = {"image": {"mean", "std", "fill"}, "midi": {"random_roll", "grayscale", "binary_thresh", "out_channels"}}[kind]
        if set(transform_kwargs) - allowed:
            raise TypeError(f"AugmentedBatches(kind={kind!r}): unexpected arguments {sorted(set(transform_kwargs) - allowed)}")
        self.pool, self.augs_per, self.batch_size, self.image_size = pool, int(augs_per), int(batch_size), N._check_aug_size(image_size)
        self.seed, self.kind, self.first_id, self.transform_kwargs = seed, kind, int(first_id), dict(transform_kwargs)
        self.items = len(pool) * self.augs_per

    def __len__(self):
        return -(-self.items // self.batch_size)

    def _host(self, lo):
        g = np.arange(lo, min(lo + self.batch_size, self.items), dtype=np.int64)
        src = g % len(self.pool)
        if self.kind == "image":
            return src, _image_host(self.pool, src, self.first_id + g, self.image_size, self.seed)
        return src, _midi_host(self.pool, src, self.first_id + g, self.image_size, self.seed, self.transform_kwargs.get("random_roll", True))

    def __iter__(self):
        import concurrent.futures
        kw = {k: v for k, v in self.transform_kwargs.items() if k != "random_roll"}
        launch = _image_launch if self.kind == "image" else _midi_launch
        with concurrent.futures.ThreadPoolExecutor(max_workers=1) as ahead:
            nxt = ahead.submit(self._host, 0)
            for lo in range(0, self.items, self.batch_size):
                src, job = nxt.result()
                if lo + self.batch_size < self.items:
                    nxt = ahead.submit(self._host, lo + self.batch_size)
                yield launch(self.pool, job, **kw), self.pool.labels[src]
