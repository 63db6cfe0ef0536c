"""The module-local references of tests/codec_taps.py, checked on the CPU oracles alone (no GPU, no native library).

(1) Wiring: with an oracle's own fp64 taps fed in as if they were the GPU's, every local reference reproduces the oracle's tap -- and the
    codec's output -- to 1e-12: both codecs, both directions, and a VQVAE with NATTEN blocks in both layouts.
(2) Sensitivity, each defect seeded on the oracle by monkeypatching:
    (a) one SD-VAE resnet normalising with eps 1e-5 where it should use 1e-6 moves the whole decode by less than the 2e-4 gate of
        tests/test_gpu_vae.py (2.5e-6), and trips exactly that resnet's rows (1.7e-5 of its branch);
    (b) one sample's attention branch scaled by 1 + 1e-4 trips exactly (that attention, that sample);
    (c) a softmax scale of (C + 8)^-1/2 trips the attention's ``.p`` rows and no other."""
import pytest
import torch
import torch.nn.functional as F

import codec_taps as ct
from conftest import load_golden, rel_l2
from oracle import sdvae_oracle as vo
from oracle import vqvae_oracle as vq
from oracle.synth import synth_input, synth_state_dict, synth_tensor


def _sd_state(seed=7):
    return {k: v.double() for k, v in ct.sdvae_weights(vo.shapes(), seed).items()}


def _vq_state(tag, natten=()):
    sd = synth_state_dict(load_golden("g9_vqvae")[tag + "_shapes"], 9)
    for n in natten:                                  # NATTENBlock parameters (codecs.py:101-105) in the blocks named, gate open
        c = sd[n + ".conv2.weight"].shape[0]
        for k, shape in ((".norm.weight", (c,)), (".norm.bias", (c,)), (".qkv.weight", (3 * c, c)), (".proj.weight", (c, c))):
            sd[n + ".attn" + k] = synth_tensor(n + ".attn" + k, shape, 4) * (1.5 if len(shape) == 2 else 1.0)
        sd[n + ".attn.gamma"] = torch.tensor([0.8])
    return {k: v.double() for k, v in sd.items()}


def _check_wiring(mods, sd, taps, x, out):
    taps = dict(taps)
    taps["x"], taps["out"] = x, out
    assert [m.name for m in mods][-1] == "out" and {m.name for m in mods} == set(taps) - {"x"}
    refs = ct.local_references(sd, taps, mods)
    for name, ref in refs.items():
        assert rel_l2(ref, taps[name]) <= 1e-12, (name, rel_l2(ref, taps[name]))
    assert ct.needed_taps(mods) == [m.name for m in mods][:-1]
    rows = ct.gate(mods, taps, refs)
    assert all(r.ok for r in rows), ct.report(rows)
    e = ct.e32(sd, taps, mods, refs64=refs)                                  # the fp32 evaluation is an fp32 evaluation: small, not zero
    assert all(0 <= m < 1e-5 for m, _ in e.values()) and max(m for m, _ in e.values()) > 1e-9, e
    return refs, e


@pytest.mark.parametrize("decode,shape", [(False, (2, 3, 64, 64)), (True, (2, 4, 8, 8)), (True, (1, 4, 16, 8))])
def test_sdvae_local_references_reproduce_the_oracles_taps(decode, shape):
    sd = _sd_state()
    x = synth_input("ct.sd", shape, 3).double() * (4.5 if decode else 1.0)
    taps = {}
    out = (vo.decode if decode else vo.encode_mean)(sd, x, taps)
    mods = ct.sd_modules(sd, decode)
    refs, e = _check_wiring(mods, sd, taps, x, out)
    a = ("decoder" if decode else "encoder") + ".mid_block.attentions.0"
    assert {a + s for s in (".q", ".k", ".v", ".p", ".o", "")} <= set(refs)
    assert ct.min_logit_std(refs[a + ".q"], refs[a + ".k"]) >= 1.0            # doubled to_q / to_k: no softmax row is flat
    print(f"\n[sd {'dec' if decode else 'enc'} {shape}] e32 per class: " + ", ".join(f"{k} {m:.1e}/{b:.1e}" for k, (m, b) in sorted(e.items())))


@pytest.mark.parametrize("tag,decode,shape,natten,layout", [
    ("gray_nd4_small", False, (3, 1, 64, 128), (), 1), ("gray_nd4_small", True, (3, 4, 4, 8), (), 1),
    ("midi_vqgan", False, (1, 3, 32, 32), (), 1), ("midi_vqgan", True, (1, 4, 4, 4), (), 1),
    ("gray_nd4_small", False, (1, 1, 128, 128), ("encoder.6", "encoder.7"), 1), ("gray_nd4_small", False, (1, 1, 128, 128), ("encoder.6",), 2),
    ("gray_nd4_small", True, (1, 4, 4, 8), ("decoder.layers.11",), 1)])
def test_vqvae_local_references_reproduce_the_oracles_taps(tag, decode, shape, natten, layout):
    sd = _vq_state(tag, natten)
    x = synth_input("ct.vq." + tag, shape, 5).double()
    if not decode:
        x = torch.sigmoid(x)
    taps = {}
    out = (vq.decode if decode else vq.encode)(sd, x, natten_layout=layout, taps=taps)
    assert rel_l2(out, (vq.decode if decode else vq.encode)(sd, x, natten_layout=layout)) == 0.0
    mods = ct.vq_modules(sd, decode, layout)
    refs, _ = _check_wiring(mods, sd, taps, x, out)
    names = set(refs)
    for n in natten:
        assert {n + ".act", n + ".qkv", n + ".att", n + ".mid"} <= names
    if decode:
        assert {"decoder.layers.0", "decoder.layers.6.q", "decoder.layers.6.p", "decoder.layers.9"} <= names
        assert rel_l2(refs["decoder.layers.9"], F.pixel_shuffle(taps["decoder.layers.7"], 2)) == 0.0
    else:
        assert {"encoder.0.res", "encoder.0.h1", "encoder.1.mid", "encoder.1.h2"} <= names and "encoder.1.res" not in names


# ---- sensitivity ---------------------------------------------------------------------------------------------------------------------
B, SHAPE = 2, (2, 4, 8, 8)


@pytest.fixture(scope="module")
def clean():
    sd = _sd_state()
    z = synth_input("ct.sens", SHAPE, 11).double() * 4.5
    return sd, z, vo.decode(sd, z)


def _bad_taps(sd, z, good):
    """The taps of a decode on the (patched) oracle, and how far its output moved."""
    bad = {}
    out = vo.decode(sd, z, bad)
    bad["x"], bad["out"] = z, out
    return bad, rel_l2(out, good)


def _gate(sd, bad):
    """Local references from the unpatched oracle (call after monkeypatch.undo()) against the patched taps."""
    mods = ct.sd_modules(sd, True)
    return ct.gate(mods, bad, ct.local_references(sd, bad, mods))


def test_a_wrong_eps_in_one_resnet_passes_the_whole_decode_gate_and_trips_that_resnet(monkeypatch, clean):
    sd, z, good = clean
    n = "decoder.mid_block.resnets.1"
    monkeypatch.setattr(vo, "_gn_silu", lambda sd_, m, x: F.silu(F.group_norm(x, vo.GROUPS, sd_[m + ".weight"], sd_[m + ".bias"],
                                                                               eps=1e-5 if m.startswith(n + ".") else vo.EPS)))
    bad, whole = _bad_taps(sd, z, good)
    monkeypatch.undo()
    rows = _gate(sd, bad)
    failing = {(r.tap, r.sample) for r in rows if not r.ok}
    mine = [r for r in rows if r.tap == n]
    print(f"\neps 1e-5 in {n}: whole decode moved {whole:.2e}; its rows: module {max(r.module for r in mine):.2e}, branch "
          f"{max(r.branch for r in mine):.2e}; failing {sorted(failing)}")
    assert 0 < whole < 2e-4, whole                                              # the whole-image gate of test_gpu_vae.py passes
    assert {(n, b) for b in range(B)} <= failing <= {(t, b) for t in (n, n + ".h1") for b in range(B)}, ct.report(rows)
    assert min(r.branch for r in mine) > 3 * ct.BRANCH_TOL                       # (measured 1.7e-5 of the branch, 2.3e-6 of the module output)


def test_one_samples_attention_branch_off_by_1e_4_trips_that_tap_and_sample(monkeypatch, clean):
    sd, z, good = clean
    a, base = "decoder.mid_block.attentions.0", vo.attention

    def perturbed(sd_, n, x, taps=None):
        y = base(sd_, n, x, taps)
        scale = torch.ones(B, 1, 1, 1, dtype=y.dtype)
        scale[-1] = 1 + 1e-4
        y = (y - x) * scale + x
        if taps is not None:
            taps[n] = y
        return y

    monkeypatch.setattr(vo, "attention", perturbed)
    bad, whole = _bad_taps(sd, z, good)
    monkeypatch.undo()
    rows = _gate(sd, bad)
    failing = {(r.tap, r.sample) for r in rows if not r.ok}
    assert whole > 0 and failing == {(a, B - 1)}, ct.report(rows)
    row = next(r for r in rows if (r.tap, r.sample) == (a, B - 1))
    assert abs(row.branch - 1e-4) < 1e-6
    print(f"\nwhole decode moved {whole:.2e}; {a}[{B - 1}] module {row.module:.2e}, branch {row.branch:.2e}")


def test_a_softmax_scale_of_c_plus_8_trips_the_scores(monkeypatch, clean):
    sd, z, good = clean
    a = "decoder.mid_block.attentions.0"

    def probs(q, k):
        b, c, h, w = q.shape
        s = torch.bmm(q.reshape(b, c, h * w).permute(0, 2, 1), k.reshape(b, c, h * w)) * (c + 8) ** -0.5
        return torch.softmax(s, dim=2).permute(0, 2, 1).reshape(b, h * w, h, w)

    monkeypatch.setattr(vo, "attn_probs", probs)
    bad, whole = _bad_taps(sd, z, good)
    monkeypatch.undo()
    rows = _gate(sd, bad)
    failing = {(r.tap, r.sample) for r in rows if not r.ok}
    assert failing == {(a + ".p", b) for b in range(B)}, ct.report(rows)
    worst = max(r.module for r in rows if r.tap == a + ".p")
    print(f"\nsoftmax scale (C+8)^-1/2: whole decode moved {whole:.2e}; {a}.p module {worst:.2e}")
    assert worst > 1e-4
