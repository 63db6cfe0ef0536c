"""The module-local references of tests/unet_taps.py, checked on the CPU oracle alone (no GPU, no native library).

(1) Wiring: with the oracle's own fp64 taps fed in as if they were the GPU's, every local reference reproduces the oracle's tap -- and
    the network output -- to 1e-12.  That pins the skip order, the mask injection before the down / up sampling convs, the final
    concatenation with ``init`` and the training plan's intermediate taps.
(2) Sensitivity: one sample's ``ups.1.2`` linear-attention branch off by 1e-4 relative moves the whole-batch output by less than the
    2e-5 forward gate of tests/test_gpu_unet.py, but trips the per-sample branch gate of the module-parity test."""
import pytest
import torch

import unet_taps as ut
from conftest import load_golden, rel_l2
from oracle import flow_oracle as fo
from oracle.synth import synth_input, synth_state_dict

# (golden shape table, seed, B, H, W, mask)
CASES = [("d32c102", 1, 2, 32, 32, False), ("d16c10", 2, 3, 16, 16, False), ("d8mask", 3, 2, 8, 8, True),
         ("d8mask", 3, 2, 8, 8, "ones"), ("d16c10", 2, 2, 16, 8, False)]


def _oracle_taps(tag, seed, B, H, W, mask):
    sd = {k: v.double() for k, v in synth_state_dict(load_golden("g3_unet_" + tag)["shapes"], seed).items()}
    x = synth_input(f"mp.x.{tag}.{H}x{W}", (B, 4, H, W), seed).double()
    t = torch.linspace(3.0, 990.0, B, dtype=torch.float64)
    cond = {}
    if "class_cond_mlp.0.weight" in sd:
        cond["class_cond"] = torch.arange(B) * 7 % sd["class_cond_mlp.0.weight"].shape[0]
    if mask == "ones":
        cond["mask_cond"] = torch.ones(B, 4, H, W, dtype=torch.float64)
    elif mask:
        cond["mask_cond"] = (synth_input(f"mp.m.{tag}", (B, 4, H, W), seed) > 0.3).double()
    taps = {}
    out = fo.unet_forward(sd, x, t, cond, taps=taps)
    taps["x"], taps["out"] = x, out
    temb = fo.time_embedding(sd, t, cond.get("class_cond"))                   # fp64 here: the oracle ran in fp64
    return sd, taps, temb, ut.mask_of(sd, cond)


@pytest.mark.parametrize("tag,seed,B,H,W,mask", CASES)
def test_local_references_reproduce_the_oracles_taps(tag, seed, B, H, W, mask):
    sd, taps, temb, m = _oracle_taps(tag, seed, B, H, W, mask)
    refs = ut.local_references(sd, temb, taps, m, internal=True)
    names = [mod.name for mod in ut.modules(sd, masked=m is not None)]
    assert set(names) - {"x", "out"} <= set(taps) and names[-1] == "out"
    checked = 0
    for name, ref in refs.items():
        if name in taps:
            assert rel_l2(ref, taps[name]) <= 1e-12, (name, rel_l2(ref, taps[name]))
            checked += 1
    internal = [n for n in taps if n.endswith(ut.INTERNAL)]
    assert internal and all(n in refs for n in internal)                      # the oracle's h1 / h2 taps are among the references
    assert checked == len(taps) - 1                                            # every tap but the input
    rows = ut.gate(sd, taps, refs, masked=m is not None)
    assert all(r.ok for r in rows), ut.report(rows)
    # the linear attention's internals feed its output: the .y reference closes the module as the oracle does
    p = "downs.0.2"
    y = fo._gn(sd, p + ".fn.fn.to_out.1", refs[p + ".y"], 1) + taps["downs.0.1"]
    assert rel_l2(y, taps[p]) <= 1e-12


def test_a_one_sample_branch_error_that_the_whole_batch_gate_misses_trips_the_module_gate(monkeypatch):
    """d32c102 at 32x32, B=4: the last sample's ups.1.2 branch scaled by (1 + 1e-4)."""
    sd, taps, temb, _ = _oracle_taps("d32c102", 1, 4, 32, 32, False)
    B, eps, p = 4, 1e-4, "ups.1.2"
    base = fo._prenorm_residual

    def perturbed(sd_, name, x, fn):
        y = base(sd_, name, x, fn)
        if name != p:
            return y
        scale = torch.ones(B, 1, 1, 1, dtype=y.dtype)
        scale[-1] = 1 + eps
        return (y - x) * scale + x

    monkeypatch.setattr(fo, "_prenorm_residual", perturbed)
    x, t = taps["x"], torch.linspace(3.0, 990.0, B, dtype=torch.float64)
    cls = torch.arange(B) * 7 % 102
    bad = {}
    out = fo.unet_forward(sd, x, t, {"class_cond": cls}, taps=bad)
    monkeypatch.undo()
    bad["x"], bad["out"] = x, out
    whole = rel_l2(out, taps["out"])
    assert 0 < whole < 2e-5, whole                                             # the old whole-batch gate passes
    rows = ut.gate(sd, bad, ut.local_references(sd, temb, bad))
    failing = {(r.tap, r.sample) for r in rows if not r.ok}
    assert failing == {(p, B - 1)}, ut.report(rows)                            # the new gate names the module and the sample
    row = next(r for r in rows if (r.tap, r.sample) == (p, B - 1))
    assert abs(row.branch - eps) < 1e-6
    print(f"\nwhole-batch output moved {whole:.2e}; {p}[{B - 1}] module {row.module:.2e}, branch {row.branch:.2e}")
