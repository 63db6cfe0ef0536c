"""The piano-roll kernels (csrc/pianoroll.hip) against the NumPy definitions of flocoder_amd.pianoroll, bit for bit: notes, their
order, counts and the -1 padding; the painter; the round trip; and sampled image -> notes -> MIDI file -> notes.  The definitions
themselves are held to upstream by tests/test_pianoroll_cpu.py."""
import numpy as np
import pytest
import torch

import pianoroll_ref as PR
from flocoder_amd import pianoroll as P
from flocoder_amd import smf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def assert_decodes(images, **kw):
    """Device == definition for uint8 images [B,3,H,W] (a NumPy array); returns the device result."""
    notes, counts = P.images_to_notes(torch.from_numpy(images).to(DEV), **kw)
    want_notes, want_counts = P.images_to_notes_np(images, **kw)
    assert notes.dtype == torch.int32 and counts.dtype == torch.int64
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    assert notes.shape == want_notes.shape and np.array_equal(notes.cpu().numpy(), want_notes)
    return notes, counts


def structured(h, w):
    """uint8 [3,H,W] with the corners of the scan (in strip 0, and across the strip boundary when there is one)."""
    img = np.zeros((3, h, w), dtype=np.uint8)
    img[1, 3, :] = 254                                           # a full-width green row, no red: one note or none
    img[1, 4, :6] = 100                                          # a green run at column 0 with no red
    img[0, 8, w - 1] = 255                                       # red in the last column
    img[0, 9, w - 9], img[1, 9, w - 8:] = 80, 80                 # a note running into the last column
    lo = max(0, min(w - 12, 58))
    img[0, 10, lo], img[1, 10, lo + 1:lo + 12] = 61, 61          # a run crossing a 64-column word (when W allows)
    if h > 128:
        img[0, 11, w - 3], img[1, 11, w - 2:] = 99, 99           # ... and a strip boundary: green goes on at column 0 of strip 1
        img[1, 128 + 11, :5] = 99
    img[0, 12, 20:23] = (21, 20, 19)                             # thresholds: only 21 is red
    img[1, 12, 23:26] = (21, 20, 19)
    img[:, 13, 30] = (255, 255, 255)
    img[:, 13, 31] = (21, 21, 21)
    img[:, 13, 32] = (21, 21, 20)                                # not white
    img[0, 0, :], img[0, 127, :] = 255, 255                      # the border rows are dropped
    return img


@pytest.mark.parametrize("require", [False, True])
@pytest.mark.parametrize("h,w,batch", [(128, 128, 3), (256, 72, 2), (384, 128, 1), (640, 128, 1), (128, 640, 1), (256, 256, 2)])
def test_decode_equals_definition(h, w, batch, require):
    """Random content over {0, 19, 20, 21, 254, 255} and random bytes (greens keep whatever r they drew), plus the structured image.
    256 x 72: two strips of 72 columns, T = 144 -- a partial last word and a flag restart inside a word; 128 x 640: ten words, so the
    second chunk of a row looks back for its flag; 640 x 128 crosses the separator at 512."""
    imgs = [PR.make_image(1000 + 7 * h + w + i, h, w, green_r0=False) for i in range(batch)] + [structured(h, w)]
    notes, counts = assert_decodes(np.stack(imgs), require_onsets=require)
    assert int(counts.min()) > 0


@pytest.mark.parametrize("require", [False, True])
def test_decode_grid(require):
    img = PR.decode_image("grid")
    img[:, 300, :], img[:, 428, :] = 0, 0
    img[1, 300, 5:], img[1, 428, :] = 77, 77                     # green through both halves of eight squares: 4096 columns, two
    img[0, 300, 5] = 77                                          # flag restarts, look-backs of up to 32 words behind the one red
    assert_decodes(img[None], require_onsets=require)


def test_empty_and_fullest_roll_share_a_batch():
    """No note at all next to the maximum count (alternating columns: 126 rows x 64 notes): N = 8064 and 8064 rows of -1 padding."""
    imgs = np.zeros((2, 3, 128, 128), dtype=np.uint8)
    imgs[1, 1, :, 0::2] = 255
    notes, counts = assert_decodes(imgs, require_onsets=False, separators=0)
    assert counts.tolist() == [0, 126 * 64] and notes.shape == (2, 126 * 64, 4) and bool((notes[0] == -1).all())
    none, zero = P.images_to_notes(torch.zeros(1, 3, 128, 128, dtype=torch.uint8, device=DEV), separators=0)
    assert none.shape == (1, 0, 4) and zero.tolist() == [0]


def test_max_notes_keeps_the_first_and_the_true_count():
    imgs = np.stack([PR.make_image(40 + i, 128, 128, green_r0=False) for i in range(2)])
    full, counts = assert_decodes(imgs)
    n = int(counts.min()) // 2
    notes, c2 = assert_decodes(imgs, max_notes=n)
    assert notes.shape == (2, n, 4) and torch.equal(c2, counts) and torch.equal(notes, full[:, :n])
    wide, _ = assert_decodes(imgs, max_notes=int(counts.max()) + 5)
    assert bool((wide[:, int(counts.max()):] == -1).all())
    again, _ = P.images_to_notes(torch.from_numpy(imgs).to(DEV))
    assert torch.equal(again, full)                              # the same bits run to run


def test_float_images_equal_the_to_uint8_path():
    from flocoder_amd.metrics import to_uint8
    u8 = np.stack([PR.make_image(60 + i, 256, 72, green_r0=False) for i in range(2)])
    g = torch.Generator().manual_seed(1)
    x = (torch.from_numpy(u8).float() / 255 * 1.7 - 0.6 + 0.01 * torch.randn(u8.shape, generator=g)).to(DEV)
    notes, counts = P.images_to_notes(x)
    via, via_counts = P.images_to_notes(to_uint8(x))
    assert torch.equal(counts, via_counts) and torch.equal(notes, via) and int(counts.min()) > 0
    want, want_counts = P.images_to_notes_np(x.cpu().numpy())
    assert np.array_equal(notes.cpu().numpy(), want) and np.array_equal(counts.cpu().numpy(), want_counts)


@pytest.mark.parametrize("require", [False, True])
def test_split_on_onsets(require):
    img = PR.make_image(77, 256, 72, runs=6.0, green_r0=False)
    img[:, 20, :] = 0
    img[0, 20, 4], img[1, 20, 5:8], img[0, 20, 8], img[1, 20, 9:12], img[0, 20, 12] = 200, 200, 100, 100, 90    # R G G G R G G G R
    merged, c0 = assert_decodes(img[None], require_onsets=require)
    split, c1 = assert_decodes(img[None], require_onsets=require, split_on_onsets=True)
    assert int(c1) > int(c0)
    rows = [r for r in split[0].cpu().tolist() if r[0] == 107 and r[1] < 20]
    assert rows == [[107, 4, 8, 100], [107, 8, 12, 50], [107, 12, 13, 45]]


def random_notes(seed, n, columns, vmin=1):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, columns - 1, size=n)
    return np.stack([rng.integers(0, 128, size=n), s, s + rng.integers(1, 40, size=n), rng.integers(vmin, 128, size=n)], axis=1).astype(np.int32)


@pytest.mark.parametrize("width", [72, 2048])
def test_painter_equals_definition(width):
    """Same-pitch overlaps in list order (pitches drawn from 128 over hundreds of notes, and the 9 / 10 / 11 neighbours), col0 > 0 with the
    onset decided by the column in front of the window, padding past the counts ignored."""
    lists = [np.concatenate([PR.paint_notes().astype(np.int32), random_notes(5, 300, 230)]), random_notes(6, 900, width + 100, vmin=5)]
    col0 = [13, 37]
    counts = np.array([len(x) for x in lists], dtype=np.int64)
    notes = np.full((2, int(counts.max()) + 3, 4), -1, dtype=np.int32)
    for i, x in enumerate(lists):
        notes[i, :len(x)] = x
    notes[0, len(lists[0]):] = (60, 0, 5000, 127)                # behind the count: must not be painted
    dn, dc = torch.from_numpy(notes).to(DEV), torch.from_numpy(counts).to(DEV)
    for c0 in (None, col0):
        got = P.notes_to_images(dn, dc, width, col0=c0).cpu().numpy()
        want = np.stack([P.notes_to_image_np(lists[i], width, 0 if c0 is None else c0[i]) for i in range(2)])
        assert got.shape == (2, 3, 128, width) and got.dtype == np.uint8 and np.array_equal(got, want)


def test_round_trip_notes_image_notes():
    """Notes with v >= 11 and a gap of at least one column per pitch come back unchanged (pitches 1..126: rows 0 and 127 are dropped)."""
    rng = np.random.default_rng(11)
    lists = []
    for width in (640, 640):
        rows = []
        for p in range(1, 127):
            t = int(rng.integers(0, 3))
            while t < width - 2:
                e = min(width, t + int(rng.integers(1, 30)))
                rows.append((p, t, e, int(rng.integers(11, 128))))
                t = e + int(rng.integers(1, 40))
        rows.sort(key=lambda r: (r[2], r[0]))
        lists.append(np.asarray(rows, dtype=np.int32))
    counts = torch.tensor([len(x) for x in lists], dtype=torch.int64, device=DEV)
    notes = torch.full((2, int(counts.max()), 4), -1, dtype=torch.int32)
    for i, x in enumerate(lists):
        notes[i, :len(x)] = torch.from_numpy(x)
    notes = notes.to(DEV)
    img = P.notes_to_images(notes, counts, 640)
    back, back_counts = P.images_to_notes(img, require_onsets=True, separators=0)
    assert torch.equal(back_counts, counts) and torch.equal(back, notes)


def test_sampled_images_to_midi_files_and_back(tmp_path):
    """A synthetic VQVAE's decode -> g2rgb (what sampler(..., is_midi=True) returns) -> notes -> .mid -> read_midi: the same notes."""
    from conftest import load_golden
    from flocoder_amd.codecs import VQVAE
    from flocoder_amd.sampling import decode_latents
    from oracle.synth import synth_input, synth_state_dict
    cfg = dict(in_channels=1, hidden_channels=32, num_downsamples=4, internal_dim=32, vq_embedding_dim=4)
    codec = VQVAE(**cfg).eval()
    codec.load_state_dict(synth_state_dict(load_golden("g9_vqvae")["gray_nd4_small_shapes"], 9), strict=False)
    codec = codec.to(DEV)
    z = synth_input("g14.z", (2, 4, 8, 8), 14).to(DEV)
    images = decode_latents(codec, z, is_midi=True)
    assert images.shape == (2, 3, 128, 128) and images.dtype == torch.float32
    notes, counts = P.images_to_notes(images, require_onsets=False)
    want, want_counts = P.images_to_notes_np(images.cpu().numpy(), require_onsets=False)
    assert np.array_equal(notes.cpu().numpy(), want) and np.array_equal(counts.cpu().numpy(), want_counts) and int(counts.min()) > 0
    paths = P.images_to_midi_files(images, tmp_path / "midi", "sample")
    assert [p.split("/")[-1] for p in paths] == ["sample_0000.mid", "sample_0001.mid"]
    for i, path in enumerate(paths):
        sec, info = smf.read_midi(path)
        assert np.array_equal(smf.quantise_notes(sec, 8), want[i, :want_counts[i]])
    from PIL import Image
    png = tmp_path / "roll.png"
    u8 = (images[0].clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
    Image.fromarray(u8, "RGB").save(png)
    mid = P.img_file_2_midi_file(str(png), output_dir=str(tmp_path), require_onsets=False)
    assert mid == str(tmp_path / "roll.mid")
    seq = P.img2midi_multi(Image.open(png), require_onsets=False)
    assert np.array_equal(smf.quantise_notes(smf.read_midi(mid)[0], 8), seq.notes)
