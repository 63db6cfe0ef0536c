"""Standard MIDI Files in pure Python: the writer the piano-roll decoder ends in and a minimal reader (no ``pretty_midi``).

A note is ``(pitch, start, end, velocity)`` in piano-roll columns; a column lasts ``1 / fs`` seconds.  At the defaults (fs = 8,
120 beats per minute, 220 ticks per beat -- ``pretty_midi``'s -- a second is 440 ticks) a column is exactly 55 ticks, so write -> read
gives the columns back.
"""
from __future__ import annotations

import struct
from typing import Iterable, List, Sequence, Tuple

import numpy as np


class NoteSequence:
    """What ``img2midi_multi`` returns in place of a ``pretty_midi.PrettyMIDI``: ``notes`` int64 [n, 4] = (pitch, start, end, velocity)
    in columns, upstream's order; ``fs`` columns per second.  ``seconds()`` gives (pitch, start s, end s, velocity) rows; ``write(path)``
    a Standard MIDI File."""

    def __init__(self, notes, fs=8, program=0):
        self.notes = np.asarray(notes, dtype=np.int64).reshape(-1, 4)
        self.fs, self.program = fs, program

    def __len__(self):
        return len(self.notes)

    def seconds(self):
        return [(int(p), s / self.fs, e / self.fs, int(v)) for p, s, e, v in self.notes.tolist()]

    def get_end_time(self):
        return float(self.notes[:, 2].max()) / self.fs if len(self.notes) else 0.0

    def write(self, path, tempo=120.0, resolution=220):
        write_midi(path, self.notes, fs=self.fs, tempo=tempo, resolution=resolution, program=self.program)


def _varlen(n: int) -> bytes:
    out = [n & 0x7f]
    n >>= 7
    while n:
        out.append((n & 0x7f) | 0x80)
        n >>= 7
    return bytes(reversed(out))


def ticks_per_column(fs=8, tempo=120.0, resolution=220) -> int:
    """Ticks of one column: resolution * tempo / 60 ticks per second over fs columns per second.  Raises unless it is a whole number."""
    t = resolution * tempo / 60.0 / fs
    if t < 1 or abs(t - round(t)) > 1e-9:
        raise ValueError(f"write_midi: a column is {t} ticks at fs={fs}, tempo={tempo}, resolution={resolution}; it must be a whole number")
    return int(round(t))


def write_midi(path, notes, fs=8, tempo=120.0, resolution=220, program=0) -> None:
    """Format-1 file: a tempo track (one set-tempo, 4/4) and one instrument track on channel 0 with a program change and the notes.
    ``notes``: rows (pitch, start, end, velocity) in columns, pitch 0..127, velocity 1..127, end > start >= 0.  At one tick note-offs come
    before note-ons, so a note that starts where another of its pitch ends stays two notes."""
    notes = np.asarray(notes, dtype=np.int64).reshape(-1, 4)
    tpc = ticks_per_column(fs, tempo, resolution)
    if len(notes) and (notes[:, 0].min() < 0 or notes[:, 0].max() > 127 or notes[:, 3].min() < 1 or notes[:, 3].max() > 127 or
                       notes[:, 1].min() < 0 or (notes[:, 2] <= notes[:, 1]).any()):
        raise ValueError("write_midi: notes need 0 <= pitch <= 127, 1 <= velocity <= 127 and end > start >= 0")
    events = []                                                  # (tick, 0 off | 1 on, order, bytes)
    for i, (p, s, e, v) in enumerate(notes.tolist()):
        events.append((s * tpc, 1, i, bytes([0x90, p, v])))
        events.append((e * tpc, 0, i, bytes([0x80, p, 0])))
    events.sort(key=lambda ev: ev[:3])
    track = bytearray(b"\x00" + bytes([0xC0, program & 0x7f]))
    now = 0
    for tick, _, _, msg in events:
        track += _varlen(tick - now) + msg
        now = tick
    track += b"\x00\xff\x2f\x00"
    us = int(round(60_000_000 / tempo))
    meta = b"\x00\xff\x51\x03" + us.to_bytes(3, "big") + b"\x00\xff\x58\x04\x04\x02\x18\x08" + b"\x00\xff\x2f\x00"
    with open(path, "wb") as f:
        f.write(b"MThd" + struct.pack(">IHHH", 6, 1, 2, resolution))
        f.write(b"MTrk" + struct.pack(">I", len(meta)) + meta)
        f.write(b"MTrk" + struct.pack(">I", len(track)) + bytes(track))


def parse_midi(data: bytes):
    """The notes of a Standard MIDI File held in ``data``: formats 0 and 1, note on / off on any channel, running status, a note-on of
    velocity 0 as a note-off, the first set-tempo (120 without one); other channel messages, meta events and sysex are skipped.  A note-off
    closes the oldest open note of its (channel, pitch).  Returns ``(notes_seconds, info)``: a list of (pitch, start s, end s, velocity)
    ordered by (end tick, pitch), and ``{'resolution', 'tempo', 'format', 'ticks'}`` with ``ticks`` the same notes as int64 [n, 4]
    (pitch, start tick, end tick, velocity)."""
    if data[:4] != b"MThd":
        raise ValueError("read_midi: not a Standard MIDI File")
    hlen, fmt, ntrk, div = struct.unpack(">IHHH", data[4:14])
    if fmt not in (0, 1):
        raise ValueError(f"read_midi: format {fmt} is not supported (0 and 1 are)")
    if div & 0x8000:
        raise ValueError("read_midi: SMPTE time division is not supported")
    pos = 8 + hlen
    tempo_us = None
    out = []
    for _ in range(ntrk):
        if data[pos:pos + 4] != b"MTrk":
            raise ValueError("read_midi: missing track chunk")
        end = pos + 8 + struct.unpack(">I", data[pos + 4:pos + 8])[0]
        pos += 8
        tick, status, open_notes = 0, None, {}
        while pos < end:
            delta = 0
            while True:
                c = data[pos]
                pos += 1
                delta = (delta << 7) | (c & 0x7f)
                if not c & 0x80:
                    break
            tick += delta
            c = data[pos]
            if c == 0xff:                                        # meta: type, length, data
                kind = data[pos + 1]
                pos += 2
                n = 0
                while True:
                    c = data[pos]
                    pos += 1
                    n = (n << 7) | (c & 0x7f)
                    if not c & 0x80:
                        break
                if kind == 0x51 and n == 3 and tempo_us is None:
                    tempo_us = int.from_bytes(data[pos:pos + 3], "big")
                pos += n
                status = None
                continue
            if c in (0xf0, 0xf7):                                # sysex: length, data
                pos += 1
                n = 0
                while True:
                    c = data[pos]
                    pos += 1
                    n = (n << 7) | (c & 0x7f)
                    if not c & 0x80:
                        break
                pos += n
                status = None
                continue
            if c & 0x80:
                status = c
                pos += 1
            elif status is None:
                raise ValueError("read_midi: data byte without a running status")
            hi = status & 0xf0
            nargs = 1 if hi in (0xC0, 0xD0) else 2
            args = data[pos:pos + nargs]
            pos += nargs
            if hi == 0x90 and args[1] > 0:
                open_notes.setdefault((status & 0x0f, args[0]), []).append((tick, args[1]))
            elif hi == 0x80 or hi == 0x90:
                stack = open_notes.get((status & 0x0f, args[0]))
                if stack:
                    t0, vel = stack.pop(0)
                    out.append((args[0], t0, tick, vel))
        pos = end
    out.sort(key=lambda n: (n[2], n[0]))
    tempo = 60_000_000 / tempo_us if tempo_us else 120.0
    sec = 60.0 / (tempo * div)
    ticks = np.asarray(out, dtype=np.int64).reshape(-1, 4)
    return [(p, s * sec, e * sec, v) for p, s, e, v in out], {"resolution": div, "tempo": tempo, "format": fmt, "ticks": ticks}


def read_midi(path):
    """``parse_midi`` of a file: ``(notes_seconds, info)``."""
    with open(path, "rb") as f:
        return parse_midi(f.read())


def quantise_notes(notes_seconds: Iterable[Sequence[float]], fs=8) -> np.ndarray:
    """get_piano_rolls' rule (pianoroll.py:137-141): ``start = round(start fs)``, ``end = start + max(1, round((end - start) fs))`` with
    ``np.round`` (half to even); rows (pitch, start s, end s, velocity) -> int64 [n, 4] in columns, order kept."""
    rows: List[Tuple[int, int, int, int]] = []
    for p, s, e, v in notes_seconds:
        start = int(np.round(s * fs))
        rows.append((int(p), start, start + max(1, int(np.round((e - s) * fs))), int(v)))
    return np.asarray(rows, dtype=np.int64).reshape(-1, 4)
