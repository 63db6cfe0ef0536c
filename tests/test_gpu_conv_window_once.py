"""Register-fed Block-closing convolutions that stage their whole input window once, in the prologue (conv_dev.h FL_WW, conv_pipe.hip "WW").

The 32-row tile's Block-closing flavours (weights global -> registers, FL_W4) used to transform the window -- GroupNorm affine, FiLM, SiLU --
chunk by chunk inside the K loop; in the whole-window form all twelve waves put every Cin chunk into LDS, transformed, before the first
MFMA.  Values and summation order are the per-chunk form's, so results must not change by a bit.  Checked here:

  * bit-equality with the build before the change (tests/golden/window_once_parent.npz, tools/make_window_once_golden.py): the dim-32
    U-Net at 4x32x32, on a plan built for 64 rows run at B = 1 (the sample-pair tiles of the 4x4 level hold an empty second sample) and
    B = 3 (an odd last pair), and on a plan built for 3 rows (small grids: at least eight closes on the 32-row tile's whole-window form);
  * the CPU oracle at the single-forward tolerance of tests/test_gpu_unet.py (rel-L2 2e-5) for a dim-16 model, whose 64-channel 4x4 closes
    have no geometry key and take the run-time-geometry whole-window flavour, and for a dim-64 model;
  * routing: the eight 8x8 / 4x4 closes of the dim-32 plan run the whole-window form of their geometry flavour and nothing else does; in
    a dim-64 model the 512-channel 4x4 closes, whose window (2 x 6 x 6 pixels x 512 channels, 166 KB) exceeds the LDS, keep the per-chunk
    loader while its 128- and 256-channel closes take the whole-window form.
"""
import pytest
import torch

from conftest import load_golden, rel_l2
from unet_taps import worst_sample
from oracle import flow_oracle as fo
from test_gpu_conv_fin_geom import _routes
from tools import make_window_once_golden as mk

pytestmark = pytest.mark.gpu
FWD_TOL = 2e-5
DEV = "cuda:0"
FL_FIN, FL_W4, FL_WW = 1, 4096, 8192
LOW_RES_CLOSES = ("downs.2.0", "downs.2.1", "downs.3.0", "downs.3.1", "mid_block1", "mid_block2", "ups.0.0", "ups.0.1")


@pytest.fixture(scope="module")
def d32():
    sd = mk.state_dict()
    x, t, cls = mk.inputs()
    out, models = {"golden": load_golden("window_once_parent")}, {}
    for rows, B in mk.CASES:
        if rows not in models:                 # (a reservation only grows: one model per plan size)
            models[rows] = mk.build_model(sd, DEV)
            models[rows].reserve(rows, mk.H, mk.W)
        m = models[rows]
        assert m.reserved_rows() == rows
        out[(rows, B)] = mk.forward(m, x, t, cls, B, DEV).cpu()
        assert m.fused_tail_errors() == 0
        out[("routes", rows, B)] = _routes(m, B)
    return out


@pytest.mark.parametrize("rows,B", mk.CASES)
def test_equals_the_build_before_whole_window_staging(d32, rows, B):
    assert torch.equal(d32[(rows, B)], torch.from_numpy(d32["golden"][f"v_rows{rows}_B{B}"]))


@pytest.mark.parametrize("B", [1, 3])
def test_the_low_resolution_closes_of_the_dim32_plan_stage_their_window_once(d32, B):
    routes = d32[("routes", 64, B)]
    ww = [r for r in routes if r[2][9] & FL_WW]
    assert sorted(r[0] for r in ww) == sorted(LOW_RES_CLOSES), [(r[0], r[1]) for r in ww]
    for module, kernel, targs in ww:
        assert kernel.endswith("+fin") and (targs[9] & FL_FIN) and (targs[9] & FL_W4) and targs[11] != 0, (module, kernel, targs)


def test_the_three_row_plan_stages_whole_windows_too(d32):
    ww = [r for r in d32[("routes", 3, 3)] if r[2][9] & FL_WW]
    assert len(ww) >= 8 and all(r[1].endswith("+fin") for r in ww), [(r[0], r[1]) for r in d32[("routes", 3, 3)]]


def _oracle_check(m, sd, x, t, cls):
    ref = fo.unet_forward(sd, x, t, {"class_cond": cls})
    for B in (1, 3):
        a = mk.forward(m, x, t, cls, B, DEV)
        e1, e2 = rel_l2(a.cpu(), ref[:B]), worst_sample(a, ref[:B])
        print(f"B={B}: rel-L2 {e1:.3e}, worst sample {e2:.3e}")
        assert e1 < FWD_TOL and e2 < FWD_TOL, (B, e1, e2)
    assert m.fused_tail_errors() == 0


def test_run_time_geometry_closes_against_the_oracle():
    """dim 16 at 4x32x32: 64 channels at 4x4 are 16 per group on the pair tile (downs.3) -- no geometry key, the run-time-geometry
    whole-window flavour; 128 channels at 4x4 (mid, ups.0) have the dim-32 plan's geometry and its flavour."""
    from flocoder_amd.unet import Unet
    from oracle.synth import synth_input, synth_state_dict
    sd = synth_state_dict(load_golden("g3_unet_d16c10")["shapes"], 5)
    m = Unet(dim=16, dim_mults=(1, 2, 4, 8), channels=4, n_classes=10).eval()
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    m.reserve(64, 32, 32)
    x, t, cls = synth_input("window_once.x16", (3, 4, 32, 32), 5), torch.tensor([0.999, 500.5, 998.0]), torch.tensor([9, 0, 4])
    ww = [r for r in _routes(m, 3) if r[2][9] & FL_WW]
    assert any(r[2][11] == 0 for r in ww if r[0].startswith("downs.3")), [(r[0], r[2]) for r in ww]
    assert any(r[2][11] != 0 for r in ww if r[0].startswith(("mid_block", "ups.0"))), [(r[0], r[2]) for r in ww]
    _oracle_check(m, sd, x, t, cls)


def test_a_window_beyond_the_lds_keeps_the_per_chunk_loader():
    """dim 64 at 4x32x32, a plan for 4 rows (every convolution on the 32-row tile): 512 channels at 4x4 (mid, ups.0) would need 16 chunks x
    10368 bytes of window, more than the 160 KiB of LDS -- per-chunk loader; 128 channels at 8x8 (downs.2) and 256 at 4x4 (downs.3) fit."""
    from flocoder_amd.unet import Unet
    torch.manual_seed(11)
    m = Unet(dim=64, dim_mults=(1, 2, 4, 8), channels=4, n_classes=10).eval()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(DEV)
    m.reserve(4, 32, 32)
    g = torch.Generator().manual_seed(12)
    x, t, cls = torch.randn(3, 4, 32, 32, generator=g), torch.tensor([2.0, 400.0, 900.0]), torch.tensor([1, 0, 7])
    fin = [r for r in _routes(m, 3) if r[1].endswith("+fin") and r[2][9] & FL_W4]
    at_4x4 = [r for r in fin if r[0].startswith(("mid_block", "ups.0.0", "ups.0.1"))]
    assert len(at_4x4) == 4 and not any(r[2][9] & FL_WW for r in at_4x4), [(r[0], r[2]) for r in fin]
    fits = [r for r in fin if r[0].startswith(("downs.2.0", "downs.2.1", "downs.3.0", "downs.3.1"))]
    assert len(fits) == 4 and all(r[2][9] & FL_WW for r in fits), [(r[0], r[2]) for r in fin]
    _oracle_check(m, sd, x, t, cls)
