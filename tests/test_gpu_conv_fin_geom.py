"""Block-closing convolutions on their geometry flavours (conv_dev.h GEO, conv_pipe.hip FC_FIN_GEOMS).

A flavour compiles one tile geometry in -- statistics form, samples per tile, channels per group, statistics slots per group -- and is
launched for an exact match only; every other Block-closing launch runs on a kernel that reads the geometry at run time.  Checked here, on plans built for 64
rows (the tiles, and with them the geometries, are chosen when the plan is built; bench.py's are those of 64 rows at 4x32x32) and run
at B = 3 and 5, so that the two-sample tiles of the 4x4 level hold a sample beyond B:

  * bit-equality with the fused output of the build before the geometry flavours, tests/golden/fin_geom_parent_fused.npz
    (tools/make_fin_geom_golden.py), at 4x8x8, 4x16x16 and 4x32x32.  Not with the two-launch form (convolution + `finalize`,
    fc_debug_set_fused_tail(0)): on that earlier build the two forms already differ at every one of these sizes (max |difference| of these
    very forwards, B = 3 and 5: 8.9e-7 / 2.1e-6 at 4x8x8, 3.8e-6 at 4x16x16, 6.0e-6 at 4x32x32), because `finalize` sums the GroupNorm(1) partials of the final value in another order than the
    convolution's tail.  At 4x32x32 every Block-closing launch is on a geometry flavour; at the smaller sizes most geometries have none
    and run on the run-time-geometry flavour of their mask, as before;
  * the CPU oracle at the single-forward tolerance of tests/test_gpu_unet.py (rel-L2 2e-5: fp32, summation order + exp ulps);
  * routing: at 4x32x32 every Block-closing launch of the dim-32 plan is on a geometry flavour (seven keys), no other launch is; a
    dim-16 model's geometries without a flavour are on run-time-geometry kernels (key 0), never on a flavour of another geometry.  (Not on
    the all-in-one kernel: it has no register-fed form of the 32-row tile, so it would sum those layers in another order -- and slower.)
"""
import ctypes as C

import pytest
import torch

from conftest import load_golden, rel_l2
from unet_taps import worst_sample
from oracle import flow_oracle as fo
from tools import make_fin_geom_golden as mk

pytestmark = pytest.mark.gpu
FWD_TOL = 2e-5
DEV = "cuda:0"
ROWS, SIZES = mk.ROWS, mk.SIZES
FL_FIN, FL_ALL = 1, 4095


def _routes(m, B):
    """[(module, plan kernel name, template arguments of the instantiation it launched)] of the plan's convolutions."""
    from flocoder_amd import _binding as Bd
    lib = Bd.lib()
    Bd.check(lib.fc_debug_conv_routes(1))
    try:
        rows = m.profile_ops(B, repeats=1)
        torch.cuda.synchronize()
    finally:
        Bd.check(lib.fc_debug_conv_routes(0))
    n = lib.fc_debug_conv_routes_read(None, 0)
    buf = C.create_string_buffer(n + 1)
    lib.fc_debug_conv_routes_read(buf, n + 1)
    rec = [tuple(int(v) for v in l.split()) for l in buf.value.decode().splitlines()]
    convs = [r for r in rows if r["kernel"].startswith("conv_igemm")]
    # profile_ops runs the plan once (warm) and then every entry once more, in plan order
    assert len(rec) == 2 * len(convs) and rec[:len(convs)] == rec[len(convs):], (len(rec), len(convs))
    return [(c["module"], c["kernel"], r) for c, r in zip(convs, rec[len(convs):])]


@pytest.fixture(scope="module")
def d32():
    """The golden's model; outputs, routes and oracle references per latent size, computed once."""
    sd = mk.state_dict()
    m = mk.build_model(sd, DEV)
    out = {"routes": {}, "golden": load_golden("fin_geom_parent_fused")}
    for H, W in SIZES:
        x, t, cls = mk.inputs(H, W)
        m.reserve(ROWS, H, W)
        assert m.reserved_rows() == ROWS
        for B in mk.BATCHES:
            out[(H, W, B)] = mk.forward(m, x, t, cls, B, DEV)
        assert m.fused_tail_errors() == 0
        out["routes"][(H, W)] = _routes(m, 5)
        out[(H, W, "ref")] = fo.unet_forward(sd, x, t, {"class_cond": cls})
    return out


@pytest.mark.parametrize("B", [3, 5])
@pytest.mark.parametrize("H,W", SIZES)
def test_equals_the_build_before_the_flavours(d32, H, W, B):
    assert torch.equal(d32[(H, W, B)].cpu(), torch.from_numpy(d32["golden"][f"v_{H}x{W}_B{B}"]))


@pytest.mark.parametrize("B", [3, 5])
@pytest.mark.parametrize("H,W", SIZES)
def test_against_the_oracle(d32, H, W, B):
    got, ref = d32[(H, W, B)], d32[(H, W, "ref")][:B]
    err = rel_l2(got.cpu(), ref)
    assert err < FWD_TOL, f"{H}x{W} B={B}: rel-L2 {err:.3e}"
    err = worst_sample(got, ref)
    assert err < FWD_TOL, f"{H}x{W} B={B}: worst sample {err:.3e}"


def test_every_block_close_of_the_bench_plan_runs_on_a_geometry_flavour(d32):
    fin = [r for r in d32["routes"][(32, 32)] if r[1].endswith("+fin")]
    assert len(fin) == 19, [r[:2] for r in fin]
    for module, kernel, targs in fin:
        assert targs[9] != FL_ALL and (targs[9] & FL_FIN) and targs[11] != 0, (module, kernel, targs)
    assert len({(r[2][:5], r[2][11]) for r in fin}) == 7, sorted({(r[2][:5], r[2][11]) for r in fin})
    for module, kernel, targs in d32["routes"][(32, 32)]:
        if not kernel.endswith("+fin"):
            assert targs[11] == 0 and not (targs[9] != FL_ALL and targs[9] & FL_FIN), (module, kernel, targs)


def test_a_geometry_without_a_flavour_runs_on_a_run_time_geometry_kernel():
    """dim 16 at 4x32x32, 4 groups: 16 channels do not fill a column tile (downs.0, downs.1, ups.3, final_res_block), 32 channels at 8x8 are
    8 per group in 2 slots and 64 channels at 4x4 16 per group on the pair tile (downs.2, downs.3) -- no key of FC_FIN_GEOMS.  The exact-match
    routing sends them to kernels that read the geometry at run time (key 0), never to a flavour of another geometry; mid / ups.0 / ups.1 /
    ups.2 happen to have the dim-32 plan's geometries and may use its flavours.  The forward is the oracle's."""
    from flocoder_amd.unet import Unet
    from oracle.synth import synth_input, synth_state_dict
    sd = synth_state_dict(load_golden("g3_unet_d16c10")["shapes"], 2)
    m = Unet(dim=16, dim_mults=(1, 2, 4, 8), channels=4, n_classes=10).eval()
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    m.reserve(ROWS, 32, 32)
    x, t, cls = synth_input("fin_geom.x16", (5, 4, 32, 32), 2), torch.tensor([0.999, 250.0, 500.5, 751.0, 998.0]), torch.tensor([9, 0, 3, 7, 5])
    fin = [r for r in _routes(m, 5) if r[1].endswith("+fin")]
    no_key = [r for r in fin if r[0].startswith(("downs.", "ups.3", "final"))]
    assert len(no_key) >= 8 and all(r[2][11] == 0 for r in no_key), [(r[0], r[2]) for r in fin]
    ref = fo.unet_forward(sd, x, t, {"class_cond": cls})
    for B in (3, 5):
        a = mk.forward(m, x, t, cls, B, DEV)
        assert rel_l2(a.cpu(), ref[:B]) < FWD_TOL and worst_sample(a, ref[:B]) < FWD_TOL, B
    assert m.fused_tail_errors() == 0
