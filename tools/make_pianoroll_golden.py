#!/usr/bin/env python3
"""tests/golden/g14_pianoroll.npz: what the *reference's* piano-roll functions (flocoder/pianoroll.py, run from the read-only reference
tree, never copied) return for the seeded inputs of tests/pianoroll_ref.py, as recorded results only -- the yardstick of the NumPy
definitions in ``flocoder_amd.pianoroll`` (tests/test_pianoroll_cpu.py).

``pretty_midi`` and ``torchvision`` are not installed; the module only needs their names, so three tiny classes and two empty modules
of our own stand in.  ``filter_redgreen`` writes PNG files into the working directory, so everything runs in a temporary one.  Stored:

    dec_<case>_<r>   int32 [n,4]  (pitch, start, end, velocity) in columns, in the order img2midi_multi(image, require_onsets=r) lists them
    paint_image      uint8 [3,128,PAINT_COLUMNS]  get_piano_rolls (fs = 8, times = columns / 8) + piano_roll_to_img of paint_notes()

Runs in the build container only (``python tools/make_pianoroll_golden.py``, about a minute of one core: the grid is a Python pixel loop).
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("FLOCODER_REFERENCE", "/root/reference")
OUT = os.path.join(REPO, "tests", "golden", "g14_pianoroll.npz")
sys.path.insert(0, os.path.join(REPO, "tests"))

import pianoroll_ref as PR  # noqa: E402


class Note:
    def __init__(self, velocity, pitch, start, end):
        self.velocity, self.pitch, self.start, self.end = velocity, pitch, start, end


class Instrument:
    def __init__(self, program=0, name=""):
        self.program, self.name, self.notes = program, name, []


class PrettyMIDI:
    def __init__(self, *a, **k):
        self.instruments = []

    def get_end_time(self):
        return max(n.end for i in self.instruments for n in i.notes)


def import_reference_pianoroll():
    pm = types.ModuleType("pretty_midi")
    pm.Note, pm.Instrument, pm.PrettyMIDI = Note, Instrument, PrettyMIDI
    tv, tvt = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tv.transforms = tvt
    for name, mod in (("pretty_midi", pm), ("torchvision", tv), ("torchvision.transforms", tvt)):
        sys.modules.setdefault(name, mod)
    spec = importlib.util.spec_from_file_location("ref_pianoroll", os.path.join(REF, "flocoder", "pianoroll.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    from PIL import Image
    ref = import_reference_pianoroll()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        for name in PR.DECODE_CASES:
            img = Image.fromarray(np.ascontiguousarray(PR.decode_image(name).transpose(1, 2, 0)), "RGB")
            for req in (0, 1):
                midi = ref.img2midi_multi(img, require_onsets=bool(req))
                rows = [(n.pitch, round(n.start * 8), round(n.end * 8), n.velocity) for n in midi.instruments[0].notes]
                assert all(abs(n.start * 8 - r[1]) < 1e-9 and abs(n.end * 8 - r[2]) < 1e-9 for n, r in zip(midi.instruments[0].notes, rows))
                out[f"dec_{name}_{req}"] = np.asarray(rows, dtype=np.int32).reshape(-1, 4)
                print(f"{name} require_onsets={req}: {len(rows)} notes", flush=True)
        midi = PrettyMIDI()
        inst = Instrument(name="PIANO")
        inst.notes = [Note(int(v), int(p), s / 8.0, e / 8.0) for p, s, e, v in PR.paint_notes().tolist()]
        midi.instruments.append(inst)
        rolls = ref.get_piano_rolls(midi, 8, remove_leading_silence=False)
        assert rolls["PIANO"].shape == (128, PR.PAINT_COLUMNS), rolls["PIANO"].shape
        ref.piano_roll_to_img(rolls["PIANO"], tmp, "paint", "PIANO")
        png = np.asarray(Image.open(os.path.join(tmp, "paint", "paint_PIANO.png")).convert("RGB"))
        out["paint_image"] = np.ascontiguousarray(png.transpose(2, 0, 1))
        os.chdir(REPO)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
