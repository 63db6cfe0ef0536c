"""Block-opening (conv1) convolutions on geometry flavours (conv_dev.h GEO1, conv_pipe.hip FC_CONV1_GEOMS).

The first convolution of every ResnetBlock of the dim-32 inference plan at 4x32x32 -- statistics of the raw output, in the up path also the
concatenated skip and the fused res_conv output -- runs on a lean flavour that compiles its output tile's geometry in, as the Block-closing
launches do.  Values and summation order are those of the run-time-geometry flavour, so results must not change by a bit.  Checked here:

  * bit-equality with an earlier build (tests/golden/window_once_parent.npz, tools/make_window_once_golden.py): the dim-32 U-Net at
    4x32x32 on a plan built for 64 rows at B = 1 (the sample-pair tiles of the 4x4 level hold an empty second sample) and B = 3 (an odd
    last pair, partial grids) and on a plan built for 3 rows.  The forwards pass through every conv1 launch, both outputs of the up
    path's launches and both concatenated sources;
  * routing, through fc_debug_conv_routes (template argument 13 is the conv1 key; argument 12 stays the Block-closing key): on the 64-row
    plan exactly the 19 conv1 launches carry a key, on the nine (tile, mask, key) flavours of FC_CONV1_GEOMS, without a fused tail; no
    other launch gains one;
  * other widths: a dim-16 model at 4x32x32 and a dim-64 model on a 4-row plan meet the CPU oracle at the single-forward tolerance of
    tests/test_gpu_unet.py (rel-L2 2e-5), and their conv1 launches run with key 0 -- all but the ones that ARE one of the nine launches:
    the dim-16 model's mid_block1 / mid_block2 (128 -> 128 channels at 4x4 on the pair tile) are the dim-32 plan's downs.3.*, and the
    dim-64 model's downs.3.* (256 -> 256 at 4x4) its mid_block*, in every argument of the launch.  Exact-match routing cannot tell them
    apart (the Block-closing flavours have the same coincidences, tests/test_gpu_conv_fin_geom.py); asserted for them is the exact
    (tile, mask, key) triple of their own geometry, for every other conv1 launch key 0;
  * the fused linear attention (linattn_fused.hip), from the record of what launch_fast launched (fc_debug_linattn_routes_read, one line
    "C n NB TT" per launch): the four n >= 256 modules of the 64-row plan ran the kernel pairs compiled for their shapes, the dim-16
    model's three C = 16 modules the pair that reads the shape at run time (0 0) and its ups.2.2 (C = 32, n = 256: the dim-32 plan's
    downs.1.2 shape) that shape's pair -- and that model meets the oracle.
"""
import ctypes as C

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
FL_FIN, FL_RES, FL_CAT, FL_STATS, FL_ALL, FL_W4 = 1, 2, 16, 64, 4095, 4096
UP = FL_STATS | FL_CAT | FL_RES
M128, M64K2, M32K4 = (4, 1, 1, 1, 1), (2, 1, 2, 1, 1), (1, 1, 4, 1, 1)


def _key(form, TB, TW, cpg, Tst):          # conv_dev.h geo_key
    return form | ((1 if TB == 2 else 0) << 2) | ((TW.bit_length() - 1) << 3) | ((cpg.bit_length() - 1) << 6) | (Tst << 10)


PAIR, FAST = 1, 2
# module -> (tile, mask, key): the table of the 19 launches
CONV1 = {}
for mods, tile, mask, key in (
        (("downs.0.0", "downs.0.1"), M128, FL_STATS, _key(FAST, 1, 16, 8, 8)),
        (("ups.3.0", "ups.3.1", "final_res_block"), M128, UP, _key(FAST, 1, 16, 8, 8)),
        (("ups.2.0", "ups.2.1"), M128, UP, _key(FAST, 1, 16, 16, 2)),
        (("downs.1.0", "downs.1.1"), M64K2, FL_STATS, _key(FAST, 1, 16, 8, 4)),
        (("ups.1.0", "ups.1.1"), M64K2, UP, _key(FAST, 1, 8, 32, 1)),
        (("downs.2.0", "downs.2.1"), M32K4, FL_STATS | FL_W4, _key(FAST, 1, 8, 16, 2)),
        (("downs.3.0", "downs.3.1"), M32K4, FL_STATS | FL_W4, _key(PAIR, 2, 4, 32, 1)),
        (("mid_block1", "mid_block2"), M32K4, FL_STATS | FL_W4, _key(PAIR, 2, 4, 64, 2)),
        (("ups.0.0", "ups.0.1"), M32K4, UP | FL_W4, _key(PAIR, 2, 4, 64, 2))):
    for m_ in mods:
        CONV1[m_] = (tile, mask, key)
FLAVOURS = set(CONV1.values())
LA_PLAN = {"downs.0.2": (32, 1024), "downs.1.2": (32, 256), "ups.2.2": (64, 256), "ups.3.2": (32, 1024)}     # module -> (C, n)


def _la_routes(m, B):
    """[(module, plan kernel name, (C, n, NB, TT))] of the plan's fused linear attention entries: what launch_fast launched for each."""
    from flocoder_amd import _binding as Bd
    lib = Bd.lib()
    Bd.check(lib.fc_debug_conv_routes(1))
    try:
        rows = m.profile_ops(B, repeats=1)
        torch.cuda.synchronize()
    finally:
        Bd.check(lib.fc_debug_conv_routes(0))
    n = lib.fc_debug_linattn_routes_read(None, 0)
    buf = C.create_string_buffer(n + 1)
    lib.fc_debug_linattn_routes_read(buf, n + 1)
    rec = [tuple(int(v) for v in l.split()) for l in buf.value.decode().splitlines()]
    fused = [r for r in rows if r["kernel"].startswith("linattn_fused")]
    # profile_ops runs the plan once (warm) and then every entry once more, in plan order
    assert len(rec) == 2 * len(fused) and rec[:len(fused)] == rec[len(fused):], (rec, [r["module"] for r in fused])
    return [(r["module"], r["kernel"], v) for r, v in zip(fused, rec[len(fused):])]


def _is_conv1(module, kernel):
    return module in CONV1 and not kernel.endswith("+fin")


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
        out[("la", rows, B)] = _la_routes(m, B)
    return out


@pytest.mark.parametrize("rows,B", mk.CASES)
def test_equals_the_build_before_the_conv1_flavours(d32, rows, B):
    assert torch.equal(d32[(rows, B)], torch.from_numpy(d32["golden"][f"v_rows{rows}_B{B}"]))


@pytest.mark.parametrize("B", [1, 3])
def test_exactly_the_19_conv1_launches_of_the_bench_plan_carry_a_key(d32, B):
    routes = d32[("routes", 64, B)]
    assert all(len(r[2]) == 13 for r in routes), routes[0]
    keyed = [r for r in routes if r[2][12] != 0]
    assert sorted(r[0] for r in keyed) == sorted(CONV1), [(r[0], r[1]) for r in keyed]
    for module, kernel, targs in keyed:
        assert _is_conv1(module, kernel), (module, kernel)
        assert targs[9] != FL_ALL and not (targs[9] & FL_FIN) and targs[11] == 0, (module, kernel, targs)
        assert (targs[:5], targs[9], targs[12]) == CONV1[module], (module, targs)
    # every Block-closing launch keeps its own key in its own place
    assert all(r[2][11] != 0 and r[2][12] == 0 for r in routes if r[1].endswith("+fin"))


@pytest.mark.parametrize("B", [1, 3])
def test_the_attention_entries_of_the_bench_plan_launch_their_plan_shape_instantiations(d32, B):
    la = d32[("la", 64, B)]
    assert [(mod, kernel) for mod, kernel, _ in la] == [(mod, "linattn_fused+fin") for mod in ("downs.0.2", "downs.1.2", "ups.2.2", "ups.3.2")], la
    for mod, kernel, rec in la:
        Cc, n = LA_PLAN[mod]
        assert rec == (Cc, n, n // 32, n // 128), (mod, rec)


def _oracle_check(m, sd, x, t, cls):
    ref = fo.unet_forward(sd, x, t, {"class_cond": cls})
    for B in (1, 3):
        a = mk.forward(m, x, t, cls, B, DEV)
        e1, e2 = rel_l2(a.cpu(), ref[:B]), worst_sample(a, ref[:B])
        print(f"B={B}: rel-L2 {e1:.3e}, worst sample {e2:.3e}")
        assert e1 < FWD_TOL and e2 < FWD_TOL, (B, e1, e2)
    assert m.fused_tail_errors() == 0


def _check_other_width(routes, same_launch):
    """Every conv1 launch runs with key 0, except the `same_launch` modules ({module: (tile, mask, key)}), which are launches of the dim-32
    plan's table argument for argument and run on exactly that flavour.  No launch of another kind carries a conv1 key."""
    conv1 = [r for r in routes if r[0] in CONV1 and not r[1].endswith("+fin")]
    assert len(conv1) == 19, [(r[0], r[1]) for r in conv1]
    for module, kernel, targs in conv1:
        print(module, kernel, "key", targs[12])
    for module, kernel, targs in routes:
        if module in same_launch and not kernel.endswith("+fin"):
            assert (targs[:5], targs[9], targs[12]) == same_launch[module] and targs[11] == 0, (module, targs)
        else:
            assert targs[12] == 0, (module, kernel, targs)


def test_a_dim16_model_keeps_its_conv1_launches_on_run_time_geometry():
    from flocoder_amd.unet import Unet
    from oracle.synth import synth_input, synth_state_dict
    sd = synth_state_dict(load_golden("g3_unet_d16c10")["shapes"], 7)
    m = Unet(dim=16, dim_mults=(1, 2, 4, 8), channels=4, n_classes=10).eval()
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    m.reserve(64, 32, 32)
    x, t, cls = synth_input("conv1_ends.x16", (3, 4, 32, 32), 7), torch.tensor([0.999, 500.5, 998.0]), torch.tensor([9, 0, 4])
    same = (M32K4, FL_STATS | FL_W4, _key(PAIR, 2, 4, 32, 1))         # 128 -> 128 channels at 4x4: the dim-32 plan's downs.3.*
    _check_other_width(_routes(m, 3), {"mid_block1": same, "mid_block2": same})
    # its n >= 256 attention modules with C = 16 (32x32 and 16x16) launch the fused pair that reads the shape at run time; ups.2.2 works
    # on 32 channels at 16x16, which IS the dim-32 plan's downs.1.2 shape, and launches that shape's pair
    la = _la_routes(m, 3)
    assert [(mod, rec) for mod, _, rec in la] == [("downs.0.2", (16, 1024, 0, 0)), ("downs.1.2", (16, 256, 0, 0)), ("ups.2.2", (32, 256, 8, 2)),
                                                  ("ups.3.2", (16, 1024, 0, 0))], la
    _oracle_check(m, sd, x, t, cls)


def test_a_dim64_model_on_a_four_row_plan_keeps_its_conv1_launches_on_run_time_geometry():
    from flocoder_amd.unet import Unet
    torch.manual_seed(13)
    m = Unet(dim=64, dim_mults=(1, 2, 4, 8), channels=4, n_classes=10).eval()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(DEV)
    m.reserve(4, 32, 32)
    g = torch.Generator().manual_seed(14)
    x, t, cls = torch.randn(3, 4, 32, 32, generator=g), torch.tensor([2.0, 400.0, 900.0]), torch.tensor([1, 0, 7])
    same = (M32K4, FL_STATS | FL_W4, _key(PAIR, 2, 4, 64, 2))         # 256 -> 256 channels at 4x4: the dim-32 plan's mid_block*
    _check_other_width(_routes(m, 3), {"downs.3.0": same, "downs.3.1": same})
    _oracle_check(m, sd, x, t, cls)
