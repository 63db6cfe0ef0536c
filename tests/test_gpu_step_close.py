"""The step-closing flavour of final_res_block's Block-closing launch (conv_dev.h FL_STEP): inside a replayed Euler step without CFG it
also runs final_conv, the Euler update and the next evaluation's init_conv, and fetches the next conditioning slice, so the step has no
`final_conv` / `init_conv` launch of its own.  FLOCODER_AMD_STEP_CLOSE=0 keeps the three launches; the library reads the switch at every
call, so both forms run in one process.

Plans are built for 64 rows (the tiles, and with them the flavour's key, are chosen when the plan is built; bench.py's are those of 64
rows at 4x32x32) and run at B = 1, 3 and 5.  Checked:

  * bit-equality of the two forms (2 and 3 steps), the route records of both, and the 3-step result against the CPU oracle's Euler
    trajectory at tests/test_gpu_unet.py's TRAJ_TOL;
  * three consecutive calls on one handle with different noise, class ids and step counts (3, 2, 4: the conditioning table moves and
    the graphs are dropped), each against the same call on a fresh handle with the switch off -- a stale conditioning slice or counter
    shows here, identical inputs would hide it;
  * the state left behind: a forward on the handle after a step-closed integration equals a fresh handle's;
  * the fall-backs (dim 16, 4x16x16 latents, CFG, a mask-conditioned model, one step, a shared device) run the three launches and give
    the switch-off run's bits.
"""
import ctypes as C

import pytest
import torch

from conftest import load_golden, rel_l2
from test_gpu_unet import TRAJ_TOL
from unet_taps import worst_sample
from oracle import flow_oracle as fo
from oracle.synth import synth_input, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = 64
FL_STEP = 16384
SWITCH = "FLOCODER_AMD_STEP_CLOSE"
D32 = ("g3_unet_d32c102", 1, dict(dim=32, channels=4, n_classes=102))
D16 = ("g3_unet_d16c10", 2, dict(dim=16, channels=4, n_classes=10))


def _state_dict(spec):
    tag, seed, _ = spec
    return synth_state_dict(load_golden(tag)["shapes"], seed)


def _model(spec, sd=None, H=32, W=32, shared=None):
    from flocoder_amd.unet import Unet
    m = Unet(dim_mults=(1, 2, 4, 8), **spec[2]).eval()
    m.load_state_dict(sd if sd is not None else _state_dict(spec), strict=True)
    m = m.to(DEV)
    if shared is not None:
        m.set_shared_device(shared)
    m.reserve(ROWS, H, W)
    return m


def _euler(m, src, cls, n, cfg=0.0, mask=None):
    from flocoder_amd import sampling as S
    cond = {"class_cond": None if cls is None else cls.to(DEV)}
    if mask is not None:
        cond["mask_cond"] = mask.to(DEV)
    lat, nfe = S.euler_sampler(m, tuple(src.shape), n, cond=cond, source=src.to(DEV), cfg_strength=cfg)
    assert nfe == n
    return lat


def _record(fn):
    """fn() with the route records on -> (its result, template arguments of every pipelined-conv launch, the step-boundary launches:
    'init_conv' / 'final_conv' / 'step_close' in enqueue order)."""
    from flocoder_amd import _binding as Bd
    lib = Bd.lib()
    Bd.check(lib.fc_debug_conv_routes(1))
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        Bd.check(lib.fc_debug_conv_routes(0))
    texts = []
    for read in (lib.fc_debug_conv_routes_read, lib.fc_debug_step_routes_read):
        n = read(None, 0)
        buf = C.create_string_buffer(n + 1)
        read(buf, n + 1)
        texts.append(buf.value.decode().splitlines())
    return out, [tuple(int(v) for v in l.split()) for l in texts[0]], texts[1]


def _inputs(tag, B, H=32, W=32, n_classes=102):
    src = synth_input(tag, (B, 4, H, W), 7)
    cls = (torch.arange(B) * 37 + len(tag)) % n_classes
    return src, cls


def _assert_three_launch_form(convs, steps, n):
    assert steps.count("init_conv") == n and steps.count("final_conv") == n and "step_close" not in steps, steps
    assert not any(r[9] != 4095 and (r[9] & FL_STEP) for r in convs)


@pytest.fixture(scope="module")
def d32():
    sd = _state_dict(D32)
    return {"sd": sd, "on": _model(D32, sd), "off": _model(D32, sd)}


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_equals_the_three_launch_form(d32, monkeypatch, B, n):
    src, cls = _inputs(f"step_close.eq{B}", B)
    # a call with another step count first, so that this call's graph is captured (and its launches recorded) now
    _euler(d32["on"], src, cls, n + 2)
    got, convs, steps = _record(lambda: _euler(d32["on"], src, cls, n))
    # the first evaluation's init_conv in the call's prologue, then n step-closing launches and nothing else at the step boundary
    assert steps == ["init_conv"] + ["step_close"] * n, steps
    flagged = [r for r in convs if r[9] != 4095 and (r[9] & FL_STEP)]
    assert len(flagged) == n and all(r[:5] == (4, 1, 1, 1, 1) and r[11] != 0 for r in flagged), flagged
    monkeypatch.setenv(SWITCH, "0")
    _euler(d32["off"], src, cls, n + 2)
    ref, convs, steps = _record(lambda: _euler(d32["off"], src, cls, n))
    _assert_three_launch_form(convs, steps, n)
    assert torch.equal(got, ref)
    assert d32["on"].fused_tail_errors() == 0 and d32["off"].fused_tail_errors() == 0
    if n == 3:
        want, _ = fo.euler_sampler(d32["sd"], src, 3, cls)
        err, worst = rel_l2(got.cpu(), want), worst_sample(got, want)
        print(f"B={B}: rel-L2 {err:.3e}, worst sample {worst:.3e} against the oracle")
        assert err < TRAJ_TOL and worst < TRAJ_TOL, (err, worst)


def test_different_inputs_per_call(d32, monkeypatch):
    calls = [(3, 5), (2, 3), (4, 5)]          # (steps, B)
    inputs = [_inputs(f"step_close.call{i}", B) for i, (_, B) in enumerate(calls)]
    got = [_euler(d32["on"], src, cls, n) for (n, _), (src, cls) in zip(calls, inputs)]
    monkeypatch.setenv(SWITCH, "0")
    for (n, B), (src, cls), g in zip(calls, inputs, got):
        fresh = _model(D32, d32["sd"])
        assert torch.equal(g, _euler(fresh, src, cls, n)), (n, B)


def test_state_left_behind(d32):
    src, cls = _inputs("step_close.state", 3)
    _euler(d32["on"], src, cls, 3)
    x, t = synth_input("step_close.fwd", (3, 4, 32, 32), 7).to(DEV), torch.tensor([0.999, 500.5, 998.0], device=DEV)
    with torch.no_grad():
        a = d32["on"](x, t, {"class_cond": cls.to(DEV)})
        b = _model(D32, d32["sd"])(x, t, {"class_cond": cls.to(DEV)})
    assert torch.equal(a, b)


def _fallback(monkeypatch, m, src, cls, n, strict=False, **kw):
    """`strict`: the plan is the launch-per-layer one, so the record must hold the step's own init_conv and final_conv launches (a small
    model's plan may be the one-workgroup-per-sample kernel, which has neither)."""
    _euler(m, src, cls, n + 2, **kw)
    got, convs, steps = _record(lambda: _euler(m, src, cls, n, **kw))
    if strict:
        _assert_three_launch_form(convs, steps, n)
    assert "step_close" not in steps and not any(r[9] != 4095 and (r[9] & FL_STEP) for r in convs)
    monkeypatch.setenv(SWITCH, "0")
    assert torch.equal(got, _euler(m, src, cls, n, **kw))


def test_fallback_dim16(monkeypatch):
    src, cls = _inputs("step_close.d16", 3, n_classes=10)
    _fallback(monkeypatch, _model(D16), src, cls, 2)


def test_fallback_16x16_latents(d32, monkeypatch):
    src, cls = _inputs("step_close.16x16", 3, 16, 16)
    _fallback(monkeypatch, _model(D32, d32["sd"], 16, 16), src, cls, 2)


def test_fallback_cfg(d32, monkeypatch):
    src, cls = _inputs("step_close.cfg", 3)
    _fallback(monkeypatch, d32["on"], src, cls, 2, strict=True, cfg=3.0)


def test_fallback_mask_conditioned_model(monkeypatch):
    spec = ("g3_unet_d8mask", 3, dict(dim=8, channels=4, n_classes=0, mask_cond=True))
    src = synth_input("step_close.mask", (2, 4, 32, 32), 7)
    mask = (synth_input("step_close.maskv", (2, 4, 32, 32), 7) > 0).float()
    _fallback(monkeypatch, _model(spec), src, None, 2, mask=mask)


def test_fallback_one_step(d32, monkeypatch):
    src, cls = _inputs("step_close.one", 3)
    m = d32["on"]
    got, convs, steps = _record(lambda: _euler(m, src, cls, 1))
    assert "step_close" not in steps and steps.count("final_conv") <= 1, steps
    monkeypatch.setenv(SWITCH, "0")
    assert torch.equal(got, _euler(m, src, cls, 1))


def test_fallback_shared_device(d32, monkeypatch):
    src, cls = _inputs("step_close.shared", 3)
    _fallback(monkeypatch, _model(D32, d32["sd"], shared=True), src, cls, 2, strict=True)
