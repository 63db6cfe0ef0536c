"""Piano-roll images <-> notes <-> MIDI files: ``flocoder/pianoroll.py``'s decoder (``img2midi_multi`` = ``regroup_lines`` +
``filter_redgreen`` + ``img2midi`` + ``piano_roll_to_pretty_midi``) and the painting of ``get_piano_rolls`` + ``piano_roll_to_img``
(onset style ``start``) on the device (``csrc/pianoroll.hip``), with their definitions in NumPy (the ``*_np`` functions, which need no
GPU and are what the kernels are tested against bit for bit).  DESIGN.md section 4 "Piano rolls and MIDI" states the same rules in words.

* ``images_to_notes`` -- uint8 or float images [B,3,H,W] -> ``notes`` int32 [B,N,4] = (pitch, start, end, velocity), padded with -1, in
  upstream's order (ascending end, then pitch), and ``counts`` int64 [B];
* ``notes_to_images`` -- padded notes + counts -> uint8 [B,3,128,width];
* ``img2midi_multi`` / ``img_file_2_midi_file`` -- upstream's signatures; a ``smf.NoteSequence`` stands in for ``pretty_midi.PrettyMIDI``;
* ``images_to_midi_files`` -- the loop of ``generate_samples.py:304-318`` (``require_onsets=False``) over a batch: one scan, one copy.

One deliberate deviation from upstream: a kept green pixel gives its g alone, where upstream adds r (mod 256) and clips to the
image-wide maximum of the kept channels; the two agree whenever green pixels have r = 0.  ``split_on_onsets`` has no upstream counterpart.
Not built: chords, onset style ``early``, several instruments, tempo maps, ``RandomVerticalShift`` / ``RandomBarCrop`` / ``StackPianoRolls*``.
"""
from __future__ import annotations

import os

import numpy as np

from .smf import NoteSequence, quantise_notes, read_midi, write_midi  # noqa: F401  (part of this module's interface)

THRESH = 20
LAYOUTS = ("strips", "square", "grid")
MAX_COLUMNS, MAX_WIDTH = 32768, 2048


# ------------------------------------------------------------------------------------------------ the definitions (NumPy, host)
def resolve_layout(height, width, layout="auto"):
    """``(layout, columns T, restart period)`` of an H x W image.  ``auto`` is ``regroup_lines``' choice by width: 256 -> ``square``
    (must be 256 x 256), 2048 -> ``grid`` (must be 2048 x 2048), anything else ``strips`` (H a multiple of 128).  The period is where the
    onset flag of ``filter_redgreen`` restarts: every row of the regrouped image."""
    if layout == "auto":
        layout = "square" if width == 256 else "grid" if width == 2048 else "strips"
    if layout not in LAYOUTS:
        raise ValueError(f"pianoroll: layout must be 'auto' or one of {LAYOUTS}, got {layout!r}")
    if layout == "square":
        if (height, width) != (256, 256):
            raise ValueError(f"pianoroll: the square layout is 256 x 256, got {height} x {width}")
        return layout, 512, 512
    if layout == "grid":
        if (height, width) != (2048, 2048):
            raise ValueError(f"pianoroll: the grid layout is 2048 x 2048, got {height} x {width}")
        return layout, 32768, 2048
    if height < 128 or height % 128 or width < 1:
        raise ValueError(f"pianoroll: a strips image is 128 S x W, got {height} x {width}")
    t = (height // 128) * width
    if t > MAX_COLUMNS:
        raise ValueError(f"pianoroll: {t} columns, more than {MAX_COLUMNS}")
    return layout, t, width


def to_uint8_np(x):
    """``metrics.to_uint8`` of one float image [3,H,W] in NumPy: per-image min / max, fp32, truncation (NaN: skipped by the range, 0)."""
    x = np.asarray(x, dtype=np.float32)
    mn = np.nanmin(x).astype(np.float32)
    d = np.maximum((np.nanmax(x).astype(np.float32) - mn).astype(np.float32), np.float32(1e-5))
    with np.errstate(invalid="ignore"):
        y = ((x - mn) / d).astype(np.float32) * np.float32(255)
    return np.nan_to_num(np.clip(y, 0, 255), nan=0.0).astype(np.uint8)


def regroup_np(img, layout="auto"):
    """uint8 [3,H,W] -> the roll's pixels [3,128,T] and the restart period."""
    img = np.asarray(img)
    if img.dtype != np.uint8:
        img = to_uint8_np(img)
    _, h, w = img.shape
    layout, t, period = resolve_layout(h, w, layout)
    if layout == "strips":
        return np.concatenate([img[:, i:i + 128] for i in range(0, h, 128)], axis=2), period
    parts = []
    for row in range(0, h, 256):
        for col in range(0, w, 256):
            sq = img[:, row:row + 256, col:col + 256]
            parts += [sq[:, :128], sq[:, 128:, ::-1]]
    return np.concatenate(parts, axis=2), period


def roll_np(img, require_onsets=True, separators=512, layout="auto"):
    """The velocity plane of one image: ``(v int32 [128 pitches, T], onset bool [128, T])`` after filter, border rows and separators;
    ``onset`` marks the red pixels (what ``split_on_onsets`` looks at)."""
    rgb, period = regroup_np(img, layout)
    r, g, b = (rgb[c].astype(np.int32) for c in range(3))
    red = (r > THRESH) & (g < THRESH) & (b < THRESH)
    green = (r < THRESH) & (g > THRESH) & (b < THRESH)
    white = (r > THRESH) & (g > THRESH) & (b > THRESH)
    t = r.shape[1]
    if require_onsets:
        out = np.zeros_like(r)
        on = np.zeros(128, dtype=bool)
        for x in range(t):
            if x % period == 0:
                on[:] = False
            keep = green[:, x] & on
            out[:, x] = np.where(red[:, x], r[:, x], np.where(keep, g[:, x], 0))
            on = red[:, x] | keep
    else:
        out = np.where(red, r, np.where(green | white, g, 0))
    onset = red.copy()
    for row in (0, 127):
        out[row] = 0
        onset[row] = False
    v = (out >> 1)[::-1].copy()                                  # pitch = 127 - row
    if separators > 0:
        v[35:93, separators::separators] = 30
    return v, onset[::-1].copy()


def plane_to_notes_np(v, onset=None, split_on_onsets=False):
    """``piano_roll_to_pretty_midi`` on integer columns: int64 [n,4] = (pitch, start, end, velocity), ascending (end, pitch).  A note starts
    where v > 0 behind a zero (or at column 0), ends at the next zero (or T) and carries v[start]; with ``split_on_onsets`` a red pixel
    behind a non-zero column ends the running note and starts another."""
    v = np.asarray(v)
    t = v.shape[1]
    nz = v > 0
    prev = np.concatenate([np.zeros((128, 1), dtype=bool), nz[:, :-1]], axis=1)
    start = nz & ~prev
    if split_on_onsets:
        start |= nz & onset
    nxt_zero = np.concatenate([~nz[:, 1:], np.ones((128, 1), dtype=bool)], axis=1)
    nxt_start = np.concatenate([start[:, 1:], np.zeros((128, 1), dtype=bool)], axis=1)
    last = nz & (nxt_zero | nxt_start)
    notes = []
    for p in range(128):
        s_idx, l_idx = np.nonzero(start[p])[0], np.nonzero(last[p])[0]
        assert len(s_idx) == len(l_idx)
        notes += [(p, int(s), int(l) + 1, int(v[p, s])) for s, l in zip(s_idx, l_idx)]
    notes.sort(key=lambda n: (n[2], n[0]))
    return np.asarray(notes, dtype=np.int64).reshape(-1, 4)


def images_to_notes_np(images, require_onsets=True, separators=512, layout="auto", *, max_notes=None, split_on_onsets=False):
    """The definition of ``images_to_notes`` on the host: ``(notes int32 [B,N,4] padded with -1, counts int64 [B])``."""
    lists = []
    for img in images:
        v, onset = roll_np(img, require_onsets, separators, layout)
        lists.append(plane_to_notes_np(v, onset, split_on_onsets))
    counts = np.asarray([len(n) for n in lists], dtype=np.int64)
    width = int(counts.max()) if max_notes is None and len(lists) else int(max_notes or 0)
    notes = np.full((len(lists), width, 4), -1, dtype=np.int32)
    for i, n in enumerate(lists):
        k = min(len(n), width)
        notes[i, :k] = n[:k]
    return notes, counts


def paint_np(notes, columns):
    """get_piano_rolls lines 142-148 on integer columns: int32 [128, columns].  In list order every note sets [start, end) of its pitch to
    its velocity, then column start - 1 to 0 (not at start = 0: upstream's wrap-around to the last column is not reproduced)."""
    v = np.zeros((128, columns), dtype=np.int32)
    for p, s, e, vel in np.asarray(notes, dtype=np.int64).reshape(-1, 4).tolist():
        if not 0 <= p <= 127:
            continue
        v[p, max(s, 0):max(min(e, columns), 0)] = min(max(vel, 0), 255)
        if 0 < s <= columns:
            v[p, s - 1] = 0
    return v


def notes_to_image_np(notes, width, col0=0):
    """The definition of ``notes_to_images`` for one roll: uint8 [3,128,width], the columns col0 .. col0 + width of the painted roll."""
    v = paint_np(notes, col0 + width)
    g = np.minimum(2 * v, 255)
    prev = np.concatenate([np.zeros((128, 1), dtype=np.int32), v[:, :-1]], axis=1)
    red = (v >= 11) & (prev <= 9)                                # column 0 has a zero in front
    img = np.zeros((3, 128, col0 + width), dtype=np.uint8)
    img[0] = np.where(red, g, 0)[::-1]
    img[1] = np.where(red, 0, g)[::-1]
    return img[:, :, col0:].copy()


# ------------------------------------------------------------------------------------------------ the device path
def _device_images(images, who):
    import torch
    if not torch.is_tensor(images):
        raise TypeError(f"{who}: images must be a tensor [B,3,H,W] (uint8 or float)")
    if not images.is_cuda:
        raise RuntimeError(f"flocoder_amd.pianoroll.{who} runs on MI355X (gfx950) only; there is no CPU path "
                           "(the *_np functions are the definitions, for tests)")
    if images.dim() == 3:
        images = images.unsqueeze(0)
    if images.dim() != 4 or images.shape[1] != 3 or images.shape[0] < 1:
        raise ValueError(f"{who}: images must be [B,3,H,W], got {tuple(images.shape)}")
    if images.dtype != torch.uint8:
        images = images.float()
    return images.contiguous()


def images_to_notes(images, require_onsets=True, separators=512, layout="auto", *, max_notes=None, split_on_onsets=False):
    """``img2midi_multi`` for a batch, on the device: images uint8 [B,3,H,W] (or float, read through ``metrics.to_uint8``'s stretch inside
    the kernel) -> ``(notes, counts)``: int32 [B,N,4] rows (pitch, start, end, velocity) in columns, ascending (end, pitch), padded with
    -1, and int64 [B] true counts.  ``max_notes=None`` reads the counts once (the call's one wait) and sizes N = max(counts) exactly;
    ``max_notes=n`` waits for nothing: the first n notes of every roll are written and ``counts`` still holds the true numbers."""
    import torch
    from . import _binding as B
    images = _device_images(images, "images_to_notes")
    bsz, _, h, w = images.shape
    layout, t, _ = resolve_layout(h, w, layout)
    if separators < 0:
        raise ValueError("images_to_notes: separators must be >= 0")
    if max_notes is not None and max_notes < 0:
        raise ValueError("images_to_notes: max_notes must be >= 0")
    dev = images.device
    nbytes = B.lib().fc_pianoroll_workspace_bytes(bsz, t)
    if nbytes < 0:
        raise ValueError(f"images_to_notes: {bsz} rolls of {t} columns are outside the library's limits")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(bsz, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        stream = B.current_stream(dev)
        B.check(B.lib().fc_pianoroll_scan(B.ptr(images), int(images.dtype != torch.uint8), bsz, h, w, LAYOUTS.index(layout),
                                          int(bool(require_onsets)), int(separators), int(bool(split_on_onsets)), B.ptr(ws), B.ptr(counts),
                                          stream))
        n = int(counts.max()) if max_notes is None else int(max_notes)
        notes = torch.empty(bsz, n, 4, dtype=torch.int32, device=dev)
        if n:
            B.check(B.lib().fc_pianoroll_emit(B.ptr(ws), bsz, t, B.ptr(notes), n, stream))
    return notes, counts


def notes_to_images(notes, counts, width, col0=None):
    """Paint note lists into red / green piano-roll images on the device: ``notes`` int32 [B,N,4] + ``counts`` [B] (as ``images_to_notes``
    returns them; entries past the count are not read) -> uint8 [B,3,128,width], the columns ``col0[b]`` (default 0) .. + width of each
    roll.  The onset of the window's first column is decided by the roll's true previous column, as in render-then-crop."""
    import torch
    from . import _binding as B
    if not (torch.is_tensor(notes) and torch.is_tensor(counts)):
        raise TypeError("notes_to_images: notes and counts must be tensors")
    if not (notes.is_cuda and counts.is_cuda):
        raise RuntimeError("flocoder_amd.pianoroll.notes_to_images runs on MI355X (gfx950) only; there is no CPU path "
                           "(notes_to_image_np is the definition, for tests)")
    if notes.dim() != 3 or notes.shape[2] != 4 or counts.shape != (notes.shape[0],) or notes.shape[0] < 1:
        raise ValueError(f"notes_to_images: notes [B,N,4] and counts [B], got {tuple(notes.shape)} and {tuple(counts.shape)}")
    if not 1 <= width <= MAX_WIDTH:
        raise ValueError(f"notes_to_images: 1 <= width <= {MAX_WIDTH}, got {width}")
    dev = notes.device
    bsz, n = notes.shape[0], notes.shape[1]
    notes = notes.to(torch.int32).contiguous()
    counts = counts.to(torch.int64).contiguous()
    if col0 is not None:
        col0 = torch.as_tensor(col0, device=dev).to(torch.int32).reshape(-1).contiguous()
        if col0.shape != (bsz,):
            raise ValueError(f"notes_to_images: col0 must have one entry per roll, got {tuple(col0.shape)}")
    out = torch.empty(bsz, 3, 128, width, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        B.check(B.lib().fc_pianoroll_render(B.ptr(notes) if n else None, B.ptr(counts), bsz, n, int(width), B.ptr(col0), B.ptr(out),
                                            B.current_stream(dev)))
    return out


def _as_device_images(img, device=None):
    """PIL image, array [H,W,3] or tensor [3,H,W] / [B,3,H,W] -> a device tensor [B,3,H,W]."""
    import torch
    if torch.is_tensor(img):
        return img if img.dim() == 4 else img.unsqueeze(0)
    arr = np.asarray(img.convert("RGB") if hasattr(img, "convert") else img)
    if arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError(f"pianoroll: an image array must be [H,W,3], got {arr.shape}")
    dev = device if device is not None else "cuda"
    return torch.from_numpy(np.ascontiguousarray(arr.transpose(2, 0, 1))).unsqueeze(0).to(dev)


def _sequences(notes, counts, fs=8):
    notes, counts = notes.cpu().numpy(), counts.cpu().numpy()
    return [NoteSequence(notes[i, :counts[i]], fs=fs) for i in range(len(counts))]


def img2midi_multi(img, require_onsets=True, separators=512, debug=False):
    """pianoroll.py:466-480 -- one image (PIL, [H,W,3] array or tensor [3,H,W]; may be a grid of images) -> its ``NoteSequence``."""
    images = _as_device_images(img)
    if debug:
        print(f"img2midi_multi: images {tuple(images.shape)}")
    notes, counts = images_to_notes(images[:1], require_onsets=require_onsets, separators=separators)
    return _sequences(notes, counts)[0]


def img_file_2_midi_file(img_file, output_dir='', require_onsets=True, separators=512, debug=False):
    """pianoroll.py:482-492 -- an image file -> a MIDI file of the same base name (in ``output_dir``, or the working directory)."""
    from PIL import Image
    if debug:
        print(f"Processing {img_file}", flush=True)
    midi = img2midi_multi(Image.open(img_file), require_onsets=require_onsets, separators=separators, debug=debug)
    midi_file = os.path.basename(img_file).replace('.png', '.mid')
    if output_dir is not None and output_dir != '':
        midi_file = os.path.join(output_dir, midi_file)
    midi.write(midi_file)
    return midi_file


def images_to_midi_files(images, output_dir, tag, require_onsets=False, separators=512, layout="auto"):
    """The loop of ``generate_samples.py:304-318`` over a batch of sampled images [B,3,H,W] on the device: one scan, one copy of the
    notes, ``{output_dir}/{tag}_{i:04d}.mid`` per image.  ``require_onsets=False`` is what that loop passes.  Returns the paths."""
    notes, counts = images_to_notes(_device_images(images, "images_to_midi_files"), require_onsets=require_onsets, separators=separators,
                                    layout=layout)
    os.makedirs(output_dir, exist_ok=True)
    paths = []
    for i, seq in enumerate(_sequences(notes, counts)):
        paths.append(os.path.join(output_dir, f"{tag}_{i:04d}.mid"))
        seq.write(paths[-1])
    return paths
