"""The module-local backward references of tests/unet_grad_taps.py, checked on the CPU oracle alone (no GPU, no native library).

(1) Wiring: the fp64 oracle forward with its taps' gradients retained, backpropagated from a random d(out); with the oracle's taps and
    tap gradients fed in as if they were the GPU's, every local activation-gradient reference, d(x), d(mask) and every parameter
    gradient (the time / class MLPs through d(temb) included) reproduces the oracle's autograd to 1e-12.  That pins the consumers of
    every tap (skip pops, the split of concatenated sources, final_res_block reading init, identity residuals), the mask paths and the
    conditioning path.
(2) Sensitivity: one sample's gradient at one tap (grad:downs.1.1, sample 2) off by 1e-4 relative moves every whole-tensor parameter
    gradient by less than the 2e-5 of tests/test_gpu_train.py, but trips the per-sample gate, which names that tap and that sample."""
import pytest
import torch

import unet_grad_taps as gt
import unet_taps as ut
from conftest import load_golden, rel_l2
from oracle import flow_oracle as fo
from oracle.synth import synth_input, synth_state_dict

# (golden shape table, seed, B, H, W, mask) -- the shapes of tests/test_unet_module_parity_cpu.py
CASES = [("d32c102", 1, 2, 32, 32, False), ("d16c10", 2, 3, 16, 16, False), ("d8mask", 3, 2, 8, 8, True),
         ("d8mask", 3, 2, 8, 8, "ones"), ("d16c10", 2, 2, 16, 8, False)]


def sample_scales(B):
    """Per-sample cotangent scales from 1e2 down to 1e-2: a sample's gradients differ from its batch mates' by orders of magnitude."""
    return torch.logspace(2, -2, B, dtype=torch.float64).view(B, 1, 1, 1)


def _oracle_backward(tag, seed, B, H, W, mask, hook=None):
    sd = {k: v.double().requires_grad_(True) for k, v in synth_state_dict(load_golden("g3_unet_" + tag)["shapes"], seed).items()}
    x = synth_input(f"bp.x.{tag}.{H}x{W}", (B, 4, H, W), seed).double().requires_grad_(True)
    t = torch.linspace(3.0, 990.0, B, dtype=torch.float64)
    cond, cls, m = {}, None, None
    if "class_cond_mlp.0.weight" in sd:
        cls = cond["class_cond"] = torch.arange(B) * 7 % sd["class_cond_mlp.0.weight"].shape[0]
    if mask == "ones":
        m = torch.ones(B, 4, H, W, dtype=torch.float64)
    elif mask:
        m = (synth_input(f"bp.m.{tag}", (B, 4, H, W), seed) > 0.3).double()
    if m is not None:
        m.requires_grad_(True)
        cond["mask_cond"] = m
    taps = {}
    out = fo.unet_forward(sd, x, t, cond, taps=taps)
    names = [mod.name for mod in ut.modules(sd, masked=m is not None)][:-1]
    for n in names:
        taps[n].retain_grad()
    if hook is not None:
        hook(taps)
    d_out = synth_input(f"bp.d.{tag}", tuple(out.shape), seed).double() * sample_scales(B)
    out.backward(d_out)
    got = {n: taps[n].detach() for n in names}
    got.update({"grad:" + n: taps[n].grad for n in names})
    got["x"], got["out"], got["dx"] = x.detach(), out.detach(), x.grad
    if m is not None:
        got["dmask"] = m.grad
    sd64 = {k: v.detach() for k, v in sd.items()}
    grads = {k: v.grad for k, v in sd.items()}
    temb = fo.time_embedding(sd64, t, cls)
    refs = gt.local_vjp(sd64, temb, got, gt.cotangents(sd64, got, d_out, masked=m is not None), t, cls,
                        None if m is None else m.detach(), fp32_sinusoid=False)     # the oracle ran its sinusoid in fp64
    return sd64, got, grads, refs


@pytest.mark.parametrize("tag,seed,B,H,W,mask", CASES)
def test_local_vjps_reproduce_the_oracles_autograd(tag, seed, B, H, W, mask):
    sd, got, grads, refs = _oracle_backward(tag, seed, B, H, W, mask)
    taps = [n for n in got if n.startswith("grad:")]
    assert set(refs.act) == set(taps) | {"dx"} | ({"dmask"} if mask else set())
    for name, ref in refs.act.items():
        assert rel_l2(ref, got[name]) <= 1e-12, (name, rel_l2(ref, got[name]))
    assert set(refs.params) == set(grads)
    for k, g in grads.items():
        r = refs.params[k]
        assert (r is None) == (g is None), k
        if g is not None:
            assert rel_l2(r, g) <= 1e-12, (k, rel_l2(r, g))
            assert refs.params_abs[k].shape == g.shape and bool((refs.params_abs[k] >= g.abs() * (1 - 1e-12)).all()), k
    if mask == "ones":                                  # the fusion convs are bypassed; the injections still read the mask
        assert refs.params["mask_fusion_conv.0.weight"] is None and refs.params["down_mask_fusions.0.0.weight"] is not None
    # every identity residual is a pass-through term of its input's gradient
    assert {"grad:downs.0.0", "grad:downs.0.1", "grad:mid_block1", "grad:mid_attn", "grad:ups.0.1"} <= set(refs.passthrough)
    grows, prows = gt.gate_activations(got, refs), gt.gate_params(grads_as_got(grads), refs)
    assert all(r.ok for r in grows) and all(r.ok for r in prows), gt.report(grows, prows)


def grads_as_got(grads):
    return {k: (torch.zeros(1, dtype=torch.float64) if g is None else g) for k, g in grads.items()}


def test_a_one_sample_gradient_error_that_the_whole_tensor_gate_misses_trips_the_per_sample_gate():
    """d32c102 at 32x32, B=4: the gradient reaching downs.1.1 scaled by (1 + 1e-4) in sample 2 inside the oracle's own backward."""
    B, s, eps, p = 4, 2, 1e-4, "downs.1.1"
    args = ("d32c102", 1, B, 32, 32, False)
    _, _, clean, _ = _oracle_backward(*args)

    def hook(taps):
        scale = torch.ones(B, 1, 1, 1, dtype=torch.float64)
        scale[s] = 1 + eps
        taps[p].register_hook(lambda g: g * scale)

    sd, bad, grads, refs = _oracle_backward(*args, hook=hook)
    moved = {k: rel_l2(g, clean[k]) for k, g in grads.items() if g is not None}
    worst = max(moved, key=moved.get)
    assert 0 < moved[worst] < 2e-5, (worst, moved[worst])                    # the whole-tensor gate of test_gpu_train.py passes
    grows, prows = gt.gate_activations(bad, refs), gt.gate_params(grads_as_got(grads), refs)
    assert all(r.ok for r in prows), gt.report([], prows)                     # every parameter is consistent with its (wrong) dY
    failing = {(r.tap, r.sample) for r in grows if not r.ok}
    assert failing == {("grad:" + p, s)}, gt.report(grows, prows)            # the new gate names the tap and the sample
    row = next(r for r in grows if (r.tap, r.sample) == ("grad:" + p, s))
    assert abs(row.rel - eps) < 1e-9
    print(f"\nworst whole-tensor parameter gradient moved {moved[worst]:.2e} ({worst}); grad:{p}[{s}] rel {row.rel:.2e}, "
          f"branch {row.branch:.2e}")
