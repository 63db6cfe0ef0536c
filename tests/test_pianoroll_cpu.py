"""The NumPy definitions of flocoder_amd.pianoroll against what upstream's functions returned (tests/golden/g14_pianoroll.npz, made by
tools/make_pianoroll_golden.py from the inputs of tests/pianoroll_ref.py), and the Standard MIDI File writer / reader.  No GPU."""
import numpy as np
import pytest
import torch

import pianoroll_ref as PR
from conftest import load_golden
from flocoder_amd import pianoroll as P
from flocoder_amd import smf


@pytest.fixture(scope="module")
def gold():
    return load_golden("g14_pianoroll")


@pytest.mark.parametrize("require", [False, True])
@pytest.mark.parametrize("name", list(PR.DECODE_CASES))
def test_decoder_definition_equals_upstream(gold, name, require):
    """Notes, velocities and ORDER of img2midi_multi, exactly: strips (one strip; five strips crossing the separator at 512 with flag
    restarts), the square, a sparse grid; both require_onsets modes."""
    img = PR.decode_image(name)
    notes, counts = P.images_to_notes_np(img[None], require_onsets=require)
    want = gold[f"dec_{name}_{int(require)}"]
    assert counts[0] == len(want) and len(want) > 50
    assert np.array_equal(notes[0], want)


def test_decoder_inputs_cover_the_rule():
    """The golden inputs keep r = 0 on green pixels (where upstream's r + g equals our g) and do hold thresholds' neighbours."""
    img = PR.decode_image("strips640")
    r, g, b = img.astype(int)
    assert not ((r < 20) & (g > 20) & (b < 20) & (r != 0)).any()
    assert all((img == v).any() for v in (19, 20, 21, 254, 255))
    assert ((r > 20) & (g > 20) & (b > 20)).any()
    assert P.resolve_layout(640, 128) == ("strips", 640, 128) and P.resolve_layout(256, 256)[0] == "square" and P.resolve_layout(2048, 2048)[0] == "grid"
    for bad in ((128, 256), (200, 128), (512, 2048)):
        with pytest.raises(ValueError):
            P.resolve_layout(*bad)


def test_painter_definition_equals_upstream(gold):
    """get_piano_rolls + piano_roll_to_img: overlaps in list order, and velocities 9, 10, 11 next to each other in every order."""
    notes = PR.paint_notes()
    img = P.notes_to_image_np(notes, PR.PAINT_COLUMNS)
    assert np.array_equal(img, gold["paint_image"])
    v = P.paint_np(notes, PR.PAINT_COLUMNS)
    pairs = {(int(v[p, 13]), int(v[p, 14])) for p in range(100, 109)}
    assert pairs == {(a, c) for a in (9, 10, 11) for c in (9, 10, 11)}          # v[t-1] = 10 in front of 11 is among them
    full = P.notes_to_image_np(notes, 60, col0=0)
    assert np.array_equal(P.notes_to_image_np(notes, 40, col0=14), P.notes_to_image_np(notes, 54)[:, :, 14:])   # render-then-crop
    assert np.array_equal(full, img[:, :, :60])


def test_split_on_onsets_definition():
    img = np.zeros((3, 128, 128), dtype=np.uint8)
    img[0, 10, 4], img[1, 10, 5:8], img[0, 10, 8], img[1, 10, 9:12] = 200, 200, 100, 100       # R G G G R G G G: upstream merges
    merged = P.images_to_notes_np(img[None], separators=0)[0][0]
    split = P.images_to_notes_np(img[None], separators=0, split_on_onsets=True)[0][0]
    assert merged.tolist() == [[117, 4, 12, 100]]
    assert split.tolist() == [[117, 4, 8, 100], [117, 8, 12, 50]]


def test_float_images_go_through_to_uint8():
    from flocoder_amd.metrics import to_uint8
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 3, 128, 72, generator=g) * 3 - 1
    assert np.array_equal(np.stack([P.to_uint8_np(i.numpy()) for i in x]), to_uint8(x).numpy())


def test_cpu_tensors_raise():
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.images_to_notes(torch.zeros(1, 3, 128, 128, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.notes_to_images(torch.zeros(1, 1, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int64), 16)


def test_midi_write_read_round_trip(tmp_path):
    notes, _ = P.images_to_notes_np(PR.decode_image("strips640")[None])
    notes = notes[0]
    path = tmp_path / "a.mid"
    smf.write_midi(path, notes)
    assert smf.ticks_per_column() == 55
    sec, info = smf.read_midi(path)
    assert info["resolution"] == 220 and info["tempo"] == 120.0 and info["format"] == 1
    assert np.array_equal(info["ticks"][:, [1, 2]], notes[:, [1, 2]].astype(np.int64) * 55)
    assert np.array_equal(smf.quantise_notes(sec, 8), notes)                    # same notes, same order
    seq = smf.NoteSequence(notes)
    seq.write(tmp_path / "b.mid")
    assert (tmp_path / "b.mid").read_bytes() == path.read_bytes()
    with pytest.raises(ValueError):
        smf.write_midi(tmp_path / "c.mid", [(60, 0, 1, 0)])
    with pytest.raises(ValueError):
        smf.write_midi(tmp_path / "c.mid", notes, fs=7)


def test_midi_reader_running_status_and_velocity_zero():
    """A hand-written format-0 file, 96 ticks per beat, tempo 500000 us (120): note-on 60, running-status note-on 64, a text meta and a
    sysex in between, then note-ons of velocity 0 under running status as the note-offs."""
    track = bytes([0x00, 0xff, 0x51, 0x03, 0x07, 0xa1, 0x20,          # set tempo 500000
                   0x00, 0x90, 60, 100,                               # on 60
                   0x30, 64, 90,                                      # +48: running status, on 64
                   0x00, 0xff, 0x01, 0x02, 0x68, 0x69,                # text "hi" (ends running status)
                   0x00, 0xf0, 0x02, 0x7e, 0xf7,                      # sysex
                   0x30, 0x90, 60, 0,                                 # +48: on 60 velocity 0 = off
                   0x81, 0x40, 64, 0,                                 # +192 (two-byte delta): running status, off 64
                   0x00, 0xb0, 7, 100,                                # a controller: skipped
                   0x00, 0xff, 0x2f, 0x00])
    data = b"MThd" + bytes([0, 0, 0, 6, 0, 0, 0, 1, 0, 96]) + b"MTrk" + len(track).to_bytes(4, "big") + track
    sec, info = smf.parse_midi(data)
    assert info["ticks"].tolist() == [[60, 0, 96, 100], [64, 48, 288, 90]]
    assert sec == [(60, 0.0, 0.5, 100), (64, 0.25, 1.5, 90)]
    assert smf.quantise_notes(sec, 8).tolist() == [[60, 0, 4, 100], [64, 2, 12, 90]]


def test_quantise_rounds_half_to_even():
    rows = smf.quantise_notes([(60, 0.5 / 8, 1.0 / 8, 1),      # start 0.5 -> 0; duration 0.5 -> 0 -> at least 1
                               (61, 1.5 / 8, 4.0 / 8, 2),      # start 1.5 -> 2; duration 2.5 -> 2
                               (62, 2.5 / 8, 6.0 / 8, 3),      # start 2.5 -> 2; duration 3.5 -> 4
                               (63, 3.0 / 8, 3.0 / 8, 4)], 8)  # empty -> one column
    assert rows.tolist() == [[60, 0, 1, 1], [61, 2, 4, 2], [62, 2, 6, 3], [63, 3, 4, 4]]
