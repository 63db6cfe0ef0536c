"""The ledger of the pipelined convolution's instantiation table: for every row of conv_pipe.hip build_rows() -- each its own device
code -- which case launched exactly that instantiation and compared what it computed with a high-precision reference.

GATED maps a row (the thirteen template arguments, tests/conv_table_rows.py) to the cases that gated it.  A case runs its GPU work
between fc_debug_conv_routes(1) and (0), asserts its numbers, and only then credits the rows of its route record.  Three kinds:

  (a) direct   one fc_debug_conv launch on a forced tile against F.conv2d in fp64 on the CPU, per sample (the worst sample, not a batch
               norm).  Tolerances are those of tests/test_gpu_kernels.py: output rel-L2 <= 1e-5, group mean <= 1e-4, group variance <= 1e-5,
               split-bf16 output <= 2e-5 and not bit-equal to the fp32 launch.  Shapes are the smallest the tile takes with TB = 1 where a
               lean row is wanted (several samples per tile set FL_MULTI, which only the all-in-one kernel and the 32-row tile have), else a
               batch whose last tile holds a sample beyond B; channel counts that are no multiple of the chunk or of the column tile.
  (b) plan     a small U-Net or codec forward, gated by the module-local fp64 references of tests/unet_taps.py / tests/codec_taps.py at
               their thresholds (module 2e-6, branch 3e-6 + 2^-22; codecs: codec_taps).  The U-Net cases start from the builders of
               tools/make_conv_routes_golden.py; the added ones reach what those do not, through shapes derived from the constant
               thresholds of conv_igemm.hip auto_tile() and from the geometry keys (each case says which).  A case that gates only some
               modules (the large batches) credits only the launches of those modules: plan entries and route lines are matched in order.
  (c) stamped  every case whose record has unstamped lean rows runs twice more with fc_debug_set_conv_stamps on.  The record must then
               name, launch for launch, the FL_STAMP twin of each such row, or the all-in-one kernel where the table has no twin; results
               are bit-equal to the unstamped run's; both runs stamp the same (workgroup, wave) slots; a stamped wave's first stamp is
               set, and in a single-launch case a wave's stamps do not decrease in the order the kernel takes them.  A stamped row is
               credited only when its unstamped twin was credited in the same case.

               One documented exception to bit-equality: where the record substitutes the all-in-one kernel for a REGISTER-FED row
               (FL_W4, no stamped twin), the bits differ by construction -- that kernel has no k-step-quad form of the 32-row tile and sums
               the products in one accumulation chain instead of two (conv_pipe.hip DB4_CHAINS).  Everything such a launch
               feeds differs downstream.  In that case the stamped run must pass the case's own fp64 gate instead (each stamped kernel is
               then compared with fp64 directly, from its own inputs), and the taps of the modules in front of the first substituted launch
               must still be bit-equal.

The closing test runs what has not run and asserts table == GATED | ALLOW, GATED & ALLOW == {}, and that every route line ever recorded
is a row of the table.  ALLOW (tests/conv_table_rows.py) holds only rows no caller can select, with the condition that shows it.
With -s every case prints the rows it credited and its worst errors.

Measured on one MI355X (profiles/conv_table_gate.md has every case): 183 rows gated -- 64 unstamped rows directly, 96 through plans, all 58
stamped rows as twins -- and 14 allowed.  Worst errors: direct output 2.4e-7 (split-bf16 2.9e-6), group mean 3.7e-7, variance 8.9e-8; U-Net
modules 8.8e-7, branches 6.6e-7 (stamped runs included); codec modules 8.7e-7 (split-bf16 4.6e-6); the Euler trajectory 2.7e-7.  Two
direct combinations do not exist: 2x2 at stride 2 stages a window of four times the tile's pixels, more than the lean flavours hold on
M128N32 and more than any flavour holds on M256N64 -- those 2x2 rows run the folded upsampling's stride-1 form and are gated through
plans -- and two 5x5 weight stages fit the LDS on M128N32 alone.
"""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

import unet_taps as ut
from conv_table_rows import (A_FL, ALLOW, BF3_TILES, FL_ALL, FL_CAT, FL_FIN, FL_GN1, FL_MEET, FL_POSTOP, FL_RES, FL_STAMP, FL_STATS, FL_STEP, FL_W4,
                             FL_WW, FL_XF, LEAN_TILES, TILES, all_in_one, describe, geo_key, lean, row, stamped, with_fl)
from oracle import flow_oracle as fo
from tools import make_conv_routes_golden as mk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_OUT, TOL_MEAN, TOL_VAR, TOL_SPLIT = 1e-5, 1e-4, 1e-5, 2e-5          # tests/test_gpu_kernels.py
# conv_dev.h conv_stamp / conv_pipe.hip: word ((workgroup * 8 + wave) * 16 + slot), wave < 8 -- 128 words per workgroup of the launch
STAMP_WGS = 65536
GATED = {}          # row -> [case ids]
LEDGER = {}         # case id -> {"rows": credited rows, "worst": {...}, "kind": "direct" / "plan"}
ROUTES = set()      # every route line any case recorded
_TABLE = []


def table():
    if not _TABLE:
        from flocoder_amd import _binding as B
        n = B.lib().fc_debug_conv_table_read(None, 0)
        buf = C.create_string_buffer(n + 1)
        B.lib().fc_debug_conv_table_read(buf, n + 1)
        _TABLE.extend(tuple(int(v) for v in l.split()) for l in buf.value.decode().splitlines())
    return set(_TABLE)


def record(fn):
    """fn() with the route record on -> (its result, the row of every pipelined-conv launch, in launch order)."""
    from flocoder_amd import _binding as B
    lib = B.lib()
    B.check(lib.fc_debug_conv_routes(1))
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        B.check(lib.fc_debug_conv_routes(0))
    n = lib.fc_debug_conv_routes_read(None, 0)
    buf = C.create_string_buffer(n + 1)
    lib.fc_debug_conv_routes_read(buf, n + 1)
    rows = [tuple(int(v) for v in l.split()) for l in buf.value.decode().splitlines()]
    ROUTES.update(rows)
    return out, rows


_STAMPS = []


def stamp_buffer():
    if not _STAMPS:
        _STAMPS.append(torch.zeros(STAMP_WGS * 8 * 16, dtype=torch.int64, device=DEV))
    return _STAMPS[0]


class Result:
    """What a case's run returns after its numerical assertions passed: the tensors a stamped rerun must reproduce bit for bit, the worst
    errors, `select(rows)` -> per launch of the route record whether a gated module launched it (None: all), and `before(i)` -> the
    names of the tensors produced in front of launch i of the record (None: unknown, that is none)."""
    def __init__(self, tensors, worst, select=None, before=None):
        self.tensors, self.worst, self.select, self.before = tensors, worst, select, before


def twin(r):
    """The row a launch of `r` goes to with stamps on (conv_pipe_select: the mask gains FL_STAMP; no such lean row: the all-in-one kernel)."""
    if not lean(r) or stamped(r):
        return r
    t = with_fl(r, r[A_FL] | FL_STAMP)
    return t if t in table() else all_in_one(r)


# Order in which a wave takes its phase stamps (conv_pipe.hip): accumulator waves 0 1 4 5, staging waves 0 1 [2 4 5 with a transform] 3
_ORDER = {False: (0, 1, 4, 5), True: (0, 1, 2, 4, 5, 3)}


def check_stamps(buf, single_launch):
    """-> bool tensor over (workgroup, wave) slots that hold a stamp.  A stamped wave's first stamp is set; in a single launch a wave's
    stamps do not decrease in the order it takes them (several launches share the buffer and overwrite each other's slots)."""
    s = buf.view(-1, 8, 16)                         # (compared on the device: only the verdicts and the slot map come back)
    used = (s[:, :, :6] != 0).any(-1)
    assert bool(used.any()), "no stamp written"
    assert bool((s[:, :, 0][used] != 0).all()), "a stamped wave without its first stamp"
    if single_launch:
        for staging in (False, True):
            w = s[:, 4:] if staging else s[:, :4]
            u = used[:, 4:] if staging else used[:, :4]
            seq = w[:, :, list(_ORDER[staging])][u]                  # [stamped waves, stamps in time order]
            last = seq[:, 0].clone()
            for j in range(1, seq.shape[1]):
                cur = seq[:, j]
                assert bool(((cur == 0) | (cur >= last)).all()), f"stamps decrease at position {j} ({'staging' if staging else 'accumulator'} waves)"
                last = torch.where(cur != 0, cur, last)
    return used.cpu()


def run_case(cid):
    """Run case `cid` (a), (b); then (c) when its record has unstamped lean rows.  Credits GATED."""
    from flocoder_amd import _binding as B
    kind, fn, needs, max_wgs = CASES[cid]
    assert max_wgs <= STAMP_WGS, f"{cid}: a grid of {max_wgs} workgroups does not fit the stamp buffer"
    try:
        res, rows = record(fn)
    except ValueError as e:                         # a refusal credits nothing (and the closing test then misses the rows)
        LEDGER[cid] = {"rows": set(), "worst": {"refused": str(e)}, "kind": kind}
        raise
    gated = [True] * len(rows) if res.select is None else res.select(rows)
    assert len(gated) == len(rows), (cid, len(gated), len(rows))
    credited = {r for r, g in zip(rows, gated) if g}
    assert needs <= credited, f"{cid}: not launched by a gated module: {[describe(r) for r in sorted(needs - credited)]}"
    assert credited <= table(), [r for r in credited if r not in table()]
    for r in credited:
        GATED.setdefault(r, []).append(cid)
    LEDGER[cid] = {"rows": set(credited), "worst": dict(res.worst), "kind": kind}
    todo = {r for r in credited if lean(r) and not stamped(r)}
    if not todo:
        return LEDGER[cid]
    # ---- (c) the same case twice with stamps on
    buf = stamp_buffer()
    want = [twin(r) for r in rows]
    used, stamped_res = [], None
    B.check(B.lib().fc_debug_set_conv_stamps(buf.data_ptr()))
    try:
        for _ in range(2):
            buf.zero_()
            try:
                sres, srows = record(fn)
            except ValueError as e:                 # the residency check refuses the stamped meeting launch: correct, and no stamped credit
                if "whole grid resident" not in str(e):
                    raise
                LEDGER[cid]["worst"]["stamped"] = "refused: " + str(e)
                return LEDGER[cid]
            assert srows == want, (f"{cid}: with stamps the launches went to "
                                   f"{[describe(r) for r in sorted(set(srows) - set(want))]} instead of {[describe(r) for r in sorted(set(want) - set(srows))]}")
            used.append(check_stamps(buf, single_launch=len(rows) == 1))
            stamped_res = stamped_res or sres
    finally:
        B.check(B.lib().fc_debug_set_conv_stamps(None))
    assert torch.equal(used[0], used[1]), f"{cid}: the two stamped runs stamp different (workgroup, wave) slots"
    # bit-equality with the unstamped run; past a substituted register-fed launch the stamped run's own fp64 gate (passed in fn) stands in
    subst = [i for i, r in enumerate(rows) if (r[A_FL] & FL_W4) and lean(r) and not lean(want[i])]
    names = list(res.tensors)
    if subst:
        names = [] if res.before is None else [n for n in names if n in res.before(subst[0])]
    for n in names:
        assert torch.equal(res.tensors[n], stamped_res.tensors[n]), f"{cid}: {n} differs between the stamped and the unstamped run"
    LEDGER[cid]["worst"]["stamped"] = (f"bit-equal: {len(names)} of {len(res.tensors)} tensors"
                                       + (f"; from launch {subst[0]} on (the all-in-one kernel for a register-fed row) the stamped run's own "
                                          f"gate, worst {max(stamped_res.worst.values()):.2e}" if subst else ""))
    twins = {want[i] for i, r in enumerate(rows) if gated[i] and stamped(want[i]) and r in credited}
    for r in twins:
        GATED.setdefault(r, []).append(cid + "+stamps")
    LEDGER[cid]["rows"] |= twins
    return LEDGER[cid]


# ------------------------------------------------------------------------------------------------------------- (a) direct cases
def _rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed * 7919 + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def _worst(got, ref):
    return ut.worst_sample(got, ref)


def direct(tile, ks, B, c0, cout, hw, c1=0, act=False, add=False, groups=0, split=False, stride=1):
    """-> a case function: one forced-tile launch against F.conv2d in fp64, per sample."""
    H, W = hw

    def fn():
        from flocoder_amd._ops import conv_debug
        pad = {1: 0, 2: 0, 3: 1, 5: 2}[ks]
        Hi, Wi = H * stride, W * stride
        x0 = _rnd(B, c0, Hi, Wi, seed=1)
        x1 = _rnd(B, c1, Hi, Wi, seed=2) if c1 else None
        w = _rnd(cout, c0 + c1, ks, ks, seed=3, scale=((c0 + c1) * ks * ks) ** -0.5)
        b = _rnd(cout, seed=4)
        ad = _rnd(B, cout, H, W, seed=5) if add else None
        xin = x0 if x1 is None else torch.cat([x0, x1], 1)
        pre = F.conv2d(xin.double(), w.double(), b.double(), padding=pad, stride=stride)
        ref = F.silu(pre) if act else pre
        ref = ref + ad.double() if add else ref
        kw = dict(pad=pad, stride=stride, out_act=act, groups_out=groups, tile=tile)
        args = (x0.to(DEV), w.to(DEV), b.to(DEV))
        kx = dict(x1=None if x1 is None else x1.to(DEV), add=None if ad is None else ad.to(DEV))
        out, st = conv_debug(*args, **kx, **kw, precision="bf16x3" if split else "fp32")
        worst = {"out": _worst(out, ref)}
        assert out.shape == ref.shape and worst["out"] <= (TOL_SPLIT if split else TOL_OUT), (tile, ks, worst)
        tensors = {"out": out.cpu()}
        if groups:
            mean, var = st
            yg = pre.reshape(B, groups, -1)
            worst["mean"], worst["var"] = _worst(mean, yg.mean(-1)), _worst(var, yg.var(-1, unbiased=False))
            assert worst["mean"] <= TOL_MEAN and worst["var"] <= TOL_VAR, (tile, ks, worst)
            tensors["mean"], tensors["var"] = mean.cpu(), var.cpu()
        if split:                                     # the split-bf16 instantiation must be the one that ran
            exact, _ = conv_debug(*args, **kx, **kw)
            worst["fp32"] = _worst(exact, ref)
            assert worst["fp32"] <= TOL_OUT and not torch.equal(out, exact)
        return Result(tensors, worst)
    return fn


# output extent and batch per tile: TB = 1 (one sample fills whole tiles: the lean rows' condition on the tiles above 32 rows; on the
# 32-row tile two samples per tile and an odd batch), and for the all-in-one rows several samples per tile with the last tile part empty
LEAN_SHAPE = {"M32N32K4": ((4, 4), 3), "M64N32K2": ((8, 8), 2), "M128N32": ((16, 16), 2), "M128N64": ((16, 16), 2), "M256N64": ((16, 16), 2)}
MULTI_SHAPE = {"M32N32K4": ((4, 4), 3), "M64N32K2": ((4, 4), 5), "M128N32": ((8, 8), 3), "M128N64": ((8, 8), 3), "M256N64": ((8, 8), 3),
               "M64N64K2": ((4, 4), 5)}
K1 = geo_key
CONV1_KEYS = {   # FC_CONV1_GEOMS, mask FL_STATS: (tile, key) -> (channels, H = W): four groups, the plan's geometry
    ("M128N32", K1(2, 1, 16, 8, 8)): (32, 32), ("M64N32K2", K1(2, 1, 16, 8, 4)): (32, 16), ("M32N32K4", K1(2, 1, 8, 16, 2)): (64, 8),
    ("M32N32K4", K1(1, 2, 4, 32, 1)): (128, 4), ("M32N32K4", K1(1, 2, 4, 64, 2)): (256, 4)}

CASES = {}       # id -> (kind, fn, rows the case exists for, upper bound of its largest grid)


def _wgs(tile, B, hw, cout):
    return (B * hw[0] * hw[1] // 32 + B) * ((cout + 31) // 32)


def _direct(cid, needs, tile, ks, B, c0, cout, hw, **kw):
    CASES[cid] = ("direct", direct(tile, ks, B, c0, cout, hw, **kw), set(needs), _wgs(tile, B, hw, cout))


for _t in TILES:
    _wide = _t in ("M128N64", "M256N64")
    (_hw, _B), (_mhw, _mB) = LEAN_SHAPE.get(_t, MULTI_SHAPE[_t]), MULTI_SHAPE[_t]
    # all-in-one rows: a mask no lean row has (concat at 1x1, activation at 2x2, concat + statistics + activation + addend at 3x3)
    _direct(f"1x1-all-{_t}", [row(_t, 1, FL_ALL)], _t, 1, _mB, 32, 96, _mhw, c1=16, groups=6, act=True)
    # (at stride 2 the window of the 256-row tile is 1024 pixels for every shape, more than the all-in-one kernel stages either: its 2x2
    # rows run the stride-1 parity form of the folded upsampling only -- the SD-VAE cases below)
    if _t != "M256N64":
        _direct(f"2x2-all-{_t}", [row(_t, 2, FL_ALL)], _t, 2, _mB, 48, 96, _mhw, act=True, stride=2)
    _direct(f"3x3-all-{_t}", [row(_t, 3, FL_ALL)], _t, 3, _mB, 32, 96, _mhw, c1=16, groups=6, act=True, add=True)
    if row(_t, 5, FL_ALL) not in ALLOW:             # (the others: two 5x5 weight stages exceed the LDS, conv_table_rows.ALLOW)
        _direct(f"5x5-all-{_t}", [row(_t, 5, FL_ALL)], _t, 5, _mB, 12, 40, _mhw)
    if _t in LEAN_TILES or _wide:
        _direct(f"1x1-plain-{_t}", [row(_t, 1, 0)], _t, 1, _B, 48, 96, _hw)
        _direct(f"1x1-act-{_t}", [row(_t, 1, FL_POSTOP)], _t, 1, _B, 48, 96, _hw, act=True)
        _direct(f"1x1-stats-{_t}", [row(_t, 1, FL_STATS)], _t, 1, _B, 48, 96, _hw, groups=6)
    # 2x2 stride 2 (space-to-depth): the window of a 128-row tile is 16 x 32 pixels = 2048 channel quads, twice what the lean flavours' staging
    # threads hold (conv_staging_fits, kLeanNPL), whatever the shape -- M128N32's lean 2x2 row is reached by the stride-1 parity form of the
    # folded upsampling alone, in the plan cases
    if _t in LEAN_TILES and _t != "M128N32":
        _direct(f"2x2s2-plain-{_t}", [row(_t, 2, 0)], _t, 2, _B, 48, 96, _hw, stride=2)
    if _t in LEAN_TILES:
        _direct(f"3x3-plain-{_t}", [row(_t, 3, 0)], _t, 3, _B, 48, 96, _hw)
        _direct(f"3x3-actadd-{_t}", [row(_t, 3, FL_POSTOP)], _t, 3, _B, 48, 96, _hw, act=True, add=True)
        _direct(f"3x3-stats-{_t}", [row(_t, 3, FL_STATS)], _t, 3, _B, 48, 96, _hw, groups=6)
        _direct(f"3x3-cat-stats-{_t}", [row(_t, 3, FL_STATS | FL_CAT)], _t, 3, _B, 32, 96, _hw, c1=16, groups=6)
    if _t in BF3_TILES:
        for _ks in (1, 2, 3) if _t != "M256N64" else (1, 3):
            _direct(f"{_ks}x{_ks}-bf16x3-{_t}", [row(_t, _ks, FL_ALL, 1)], _t, _ks, _mB, 72, 96, _mhw, split=True, stride=2 if _ks == 2 else 1)
# the register-fed (k-step-quad) forms of the 32-row tile: whole 32-channel chunks and column tiles
_direct("3x3-plain-w4", [row("M32N32K4", 3, FL_W4)], "M32N32K4", 3, 3, 96, 64, (4, 4))
_direct("3x3-actadd-w4", [row("M32N32K4", 3, FL_POSTOP | FL_W4)], "M32N32K4", 3, 3, 64, 64, (4, 4), act=True, add=True)
_direct("3x3-stats-w4", [row("M32N32K4", 3, FL_STATS | FL_W4)], "M32N32K4", 3, 3, 64, 64, (4, 4), groups=8)
_direct("3x3-cat-stats-w4", [row("M32N32K4", 3, FL_STATS | FL_CAT | FL_W4)], "M32N32K4", 3, 3, 32, 64, (4, 4), c1=32, groups=8)
# the conv1 geometry flavours with mask FL_STATS: four groups at the dim-32 plan's geometry (conv1_geo_key), B = 3 (odd: the pair keys)
for (_t, _key), (_c, _h) in CONV1_KEYS.items():
    _w4 = FL_W4 if _t == "M32N32K4" else 0
    _direct(f"3x3-conv1-key{_key}-{_t}", [row(_t, 3, FL_STATS | _w4, 0, 0, _key)], _t, 3, 3, _c, _c, (_h, _h), groups=4)


# ------------------------------------------------------------------------------------------------------------- (b) plan cases
def _plan_entries(model):
    from flocoder_amd import _binding as B
    out = []
    for i in range(B.lib().fc_unet_plan_launches(model._handle)):
        k, m = C.c_char_p(), C.c_char_p()
        B.check(B.lib().fc_unet_op_info(model._handle, i, C.byref(k), C.byref(m), None))
        out.append((k.value.decode(), m.value.decode()))
    return out


def unet_case(dim, B, H=32, W=32, n_classes=102, plan="exclusive", only=None, rows=mk.ROWS, **kw):
    """-> a case function: one forward of a U-Net from the builders of tools/make_conv_routes_golden.py (default-initialised at seed 0),
    every module in `only` (None: all) against its module-local fp64 reference, per sample (tests/unet_taps.py, its thresholds)."""
    def fn():
        from flocoder_amd import _binding as Bd
        from flocoder_amd._ops import fetch_tap
        train = plan == "train"
        if plan == "fused_tail_off":
            Bd.check(Bd.lib().fc_debug_set_fused_tail(0))
        try:
            model = mk._unet(dim, H, W, rows=0 if train else rows, shared={"exclusive": False, "shared": True}.get(plan),
                             n_classes=n_classes, train=train, **kw)
            x, t, cls = mk._inputs(B, H, W, n_classes)
            cond = {"class_cond": cls} if n_classes else None
            with (torch.enable_grad() if train else torch.no_grad()):
                out = model(x, t, cond).detach()
            torch.cuda.synchronize()
            assert model.fused_tail_errors() == 0
        finally:
            if plan == "fused_tail_off":
                Bd.check(Bd.lib().fc_debug_set_fused_tail(-1))
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        sd64 = {k: v.double() for k, v in sd.items()}
        mods = [m for m in ut.modules(sd64) if only is None or m.name in only]
        want = {n for m in mods for n in (m.name, *m.inputs)} - {"x", "out"}
        if train:
            want |= {m.name + s for m in mods for s in m.internal}
        got = {n: fetch_tap(model, n, B).cpu() for n in sorted(want)}
        got["x"], got["out"] = x.cpu(), out.cpu()
        ctx = ut.Ctx(sd64, ut.conditioning(sd, t.cpu(), None if cond is None else {"class_cond": cls.cpu()}), None, kw.get("resnet_block_groups", 4))
        refs = {}
        for m in mods:
            side = {}
            refs[m.name] = m.fn(ctx, torch.cat([got[n].double() for n in m.inputs], dim=1), side)
            if train:
                refs.update({k: v for k, v in side.items() if k.endswith(ut.INTERNAL)})
        gate = ut.gate(sd64, got, refs)
        assert gate and all(r.ok for r in gate), ut.report(gate)
        assert len({r.sample for r in gate}) == B
        worst = {"module": max(r.module for r in gate), "branch": max([r.branch for r in gate if r.branch == r.branch], default=0.0)}
        tensors = {n: got[n] for n in refs}
        # the plan's convolution entries and the route lines, in order: which module launched what
        order = [m.name for m in ut.modules(sd64)]
        convs = [m for k, m in _plan_entries(model) if k.startswith("conv_igemm")]

        def owners(rows):
            assert len(rows) == len(convs), f"{len(rows)} route lines for {len(convs)} convolution entries of the plan"
            return convs

        def before(i):                              # taps of the modules in front of the one that owns launch i (internal taps: their module's)
            k = order.index(convs[i]) if convs[i] in order else 0
            return {n for n in tensors if any(n == m or (n.startswith(m + ".") and n.endswith(ut.INTERNAL)) for m in order[:k])}
        return Result(tensors, worst, select=None if only is None else (lambda rows: [m in only for m in owners(rows)]),
                      before=lambda i: before(i) if len(convs) > i else set())
    return fn


def euler_case():
    """Two replayed Euler steps on the dim-32 exclusive plan (the model and inputs of mk.case_euler): the step-closing flavour.  Gated as
    tests/test_gpu_step_close.py gates it: the trajectory per sample against the CPU oracle's at TRAJ_TOL, and bit-equality with the
    three-launch form (FLOCODER_AMD_STEP_CLOSE=0, read at every call), whose final_res_block launch is the row the `exclusive` case
    gates module-locally.  Credits the FL_STEP launches only: the rest of the record is gated by the trajectory alone."""
    from flocoder_amd import sampling as S
    from test_gpu_unet import TRAJ_TOL

    def sample(switch_off):
        old = os.environ.get("FLOCODER_AMD_STEP_CLOSE")
        if switch_off:
            os.environ["FLOCODER_AMD_STEP_CLOSE"] = "0"
        try:
            m = mk._unet(32, shared=False)           # a fresh handle: its graphs are captured (and their launches recorded) now
            x, _, cls = mk._inputs(3)
            lat, nfe = S.euler_sampler(m, tuple(x.shape), 2, cond={"class_cond": cls}, source=x)
            torch.cuda.synchronize()
            assert nfe == 2 and m.fused_tail_errors() == 0
            return m, x, cls, lat
        finally:
            if switch_off:
                if old is None:
                    os.environ.pop("FLOCODER_AMD_STEP_CLOSE")
                else:
                    os.environ["FLOCODER_AMD_STEP_CLOSE"] = old

    def fn():
        m, x, cls, lat = sample(False)
        sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        want, _ = fo.euler_sampler(sd, x.cpu(), 2, cls.cpu())
        worst = {"trajectory": ut.worst_sample(lat, want)}
        assert worst["trajectory"] <= TRAJ_TOL, worst
        assert torch.equal(lat, sample(True)[3]), "the step-closing launch and the three-launch form differ"
        return Result({"latents": lat.cpu()}, worst, select=lambda rows: [lean(r) and bool(r[A_FL] & FL_STEP) for r in rows])
    return fn


def codec_case(cid, spec=None):
    """A case of tests/test_gpu_codec_module_parity.py (its codecs, inputs, taps and gate: tests/codec_taps.py at its thresholds), or
    `spec`, a case in that table's format run by the same function.  A case that gates only some modules credits only their launches."""
    def fn():
        import test_gpu_codec_module_parity as cp
        if spec is not None:
            cp.CASES[cid] = spec
        try:
            prefixes = cp.CASES[cid][4]
            mods, got, refs, gate, ops = cp.run_case(cid)
        finally:
            if spec is not None:
                cp.CASES.pop(cid, None)
                cp._SEEN.pop(cid, None)
        assert gate and all(r.ok for r in gate), cp.describe(cid, mods, gate)
        convs = [m for k, m in ops if k.startswith("conv_igemm")]

        def select(rows):
            assert len(rows) == len(convs), f"{len(rows)} route lines for {len(convs)} convolution entries of the plan"
            return [cp._under(m, prefixes) for m in convs]
        return Result({n: got[n] for n in refs if n in got}, {"module": max(r.module for r in gate)}, select=None if prefixes is None else select)
    return fn


def _plan(cid, fn, needs, wgs):
    CASES[cid] = ("plan", fn, set(needs), wgs)


FIN = FL_STATS | FL_XF | FL_FIN
M32, M64, M128 = "M32N32K4", "M64N32K2", "M128N32"
# --- the cases of tools/make_conv_routes_golden.py
_plan("exclusive", unet_case(32, 5), [row(M128, 3, FIN | FL_MEET, 0, K1(2, 1, 16, 8, 8)), row(M32, 3, FIN | FL_MEET | FL_W4 | FL_WW, 0, K1(1, 2, 4, 64, 2)),
                                      row(M64, 3, FIN, 0, K1(2, 1, 8, 32, 1)), row(M32, 3, FL_STATS | FL_CAT | FL_RES | FL_W4, 0, 0, K1(1, 2, 4, 64, 2))], 4096)
_plan("shared", unet_case(32, 5, plan="shared"), [row(M128, 3, FL_STATS | FL_XF), row(M32, 3, FL_STATS | FL_XF | FL_W4)], 4096)
_plan("dim16-32x32", unet_case(16, 3, n_classes=10), [row(M128, 3, FIN | FL_MEET)], 4096)
_plan("dim16-8x8", unet_case(16, 3, 8, 8, n_classes=10), [row(M32, 3, FIN | FL_W4 | FL_WW)], 4096)
_plan("train-16x16", unet_case(32, 4, 16, 16, plan="train"), [row(M32, 1, FL_XF), row(M32, 3, FL_STATS | FL_XF | FL_W4)], 4096)
# --- added: what those do not reach
# train-mode plans keep to_qkv as a 1x1 convolution with the GroupNorm(1) loader (Cout = 384): auto_tile() gives it, at 32x32,
# M64N32K2 at B = 2 (32 x 12 = 384 >= 256 workgroups, M128N32's 192 < 256), M128N32 at B = 3 (288), M128N64 once 8 B x 6 >= 512 (B = 11)
# and M256N64 once 4 B x 6 >= 512 (B = 22); only the two 32x32 linear attentions are gated at these sizes
_LA = ("downs.0.2", "ups.3.2")
_plan("train-32x32-B2", unet_case(32, 2, plan="train", only=_LA), [row(M64, 1, FL_XF)], 4096)
_plan("train-32x32-B3", unet_case(32, 3, plan="train", only=_LA), [row(M128, 1, FL_XF)], 4096)
_plan("train-32x32-B11", unet_case(32, 11, plan="train", only=_LA), [row("M128N64", 1, FL_XF)], 8192)
_plan("train-32x32-B22", unet_case(32, 22, plan="train", only=_LA), [row("M256N64", 1, FL_XF)], 16384)
# a shared-device dim-16 plan at 8x8: block2 of the 16-channel Blocks (transform loader + statistics, no tail) on the 32-row tile with a
# Cin that is no whole 32-channel chunk -- the LDS-fed form
_plan("dim16-8x8-shared", unet_case(16, 3, 8, 8, n_classes=10, plan="shared"), [row(M32, 3, FL_STATS | FL_XF)], 4096)
# Block-closing launches without a meeting on the 128-row tile: a sample of 16x8 pixels is one tile and eight groups of 16 channels fit
# its 32 columns (T = 1, conv_geometry fin_local); auto_tile() takes M128N32 for 128 channels once 4 B >= 256 workgroups
_plan("dim64-g8-32x16-B64", unet_case(64, 64, 32, 16, resnet_block_groups=8, only=("ups.2.0", "ups.2.1")),
      [row(M128, 3, FIN), row(M128, 3, FIN | FL_GN1)], 16384)
# eight groups at dim 32: 256 channels @ 4x4 and 128 @ 8x8 have the keys of the table's 128 @ 4x4 and 64 @ 8x8 rows (cpg 32 / 16) but not
# Cin = 4 cpg, which the whole-window form of a keyed flavour assumes (conv_pipe_select): the keyed register-fed rows WITHOUT FL_WW
_plan("dim32-g8", unet_case(32, 3, rows=8, resnet_block_groups=8),
      [row(M32, 3, FIN | FL_W4 | v, 0, K1(1, 2, 4, 32, 1)) for v in (0, FL_GN1)] + [row(M32, 3, FIN | FL_W4 | FL_MEET | v, 0, K1(2, 1, 8, 16, 2)) for v in (0, FL_GN1)], 4096)
# two groups at dim 16: 128 channels @ 4x4 in groups of 64 -- the key of the table's 256 @ 4x4 row, again without Cin = 4 cpg
_plan("dim16-g2", unet_case(16, 3, n_classes=10, resnet_block_groups=2),
      [row(M32, 3, FIN | FL_W4 | FL_MEET | v, 0, K1(1, 2, 4, 64, 2)) for v in (0, FL_GN1)], 4096)
# 512 channels @ 4x4 (dim 64): no key (TB Cin exceeds a staging thread each, fin_geo_key) and a window of 72 x 128 channel quads, more than
# the whole-window form's kWWSlots x 768 (ww_lds): the run-time-geometry register-fed rows without FL_WW -- four groups of 128 span four
# column tiles (meeting), sixteen groups of 32 one each (local)
_D3 = ("downs.3.0", "downs.3.1", "mid_block1", "mid_block2")
_plan("dim64-g4-512ch", unet_case(64, 3, rows=8, only=_D3), [row(M32, 3, FIN | FL_W4 | FL_MEET), row(M32, 3, FIN | FL_W4 | FL_MEET | FL_GN1)], 8192)
_plan("dim64-g16-512ch", unet_case(64, 3, rows=8, resnet_block_groups=16, only=_D3), [row(M32, 3, FIN | FL_W4), row(M32, 3, FIN | FL_W4 | FL_GN1)], 8192)
# 64 channels @ 8x8 on the 64-row tile (a plan of 128 rows: 2 x 128 = 256 workgroups of M64N32K2, auto_tile): a sample is one tile, four groups
# of 16 fit its columns -- the run-time-geometry Block-closing rows of that tile without a meeting
_plan("dim16-rows128", unet_case(16, 3, n_classes=10, rows=128, only=("ups.1.0", "ups.1.1")), [row(M64, 3, FIN), row(M64, 3, FIN | FL_GN1)], 4096)
_plan("euler", euler_case(), [row(M128, 3, FIN | FL_MEET | FL_STEP, 0, K1(2, 1, 16, 8, 8))], 4096)
for _c in ("sd-dec-B3-8x8", "sd-dec-B2-8x8-bf16x3", "vq-gray-dec-B3-4x8"):
    _plan("codec-" + _c, codec_case(_c), [], 8192)
# the 2x2 rows of the 256-row tile: the folded upsampling of the SD-VAE decoder's 256-channel up block at 64x64 -> 128x128, B = 2 -- four parity
# classes x 32 pixel tiles x 4 column tiles = 512 workgroups of M256N64, auto_tile()'s threshold; only that upsampler is gated
_UP = ("decoder.up_blocks.2.upsamplers.0",)
_plan("codec-sd-dec-B2-16x16-up", codec_case("table-sd-dec-B2-16x16-up", ("sd", True, (2, 4, 16, 16), "fp32", _UP, set())), [row("M256N64", 2, FL_ALL)], 8192)
_plan("codec-sd-dec-B2-16x16-up-bf16x3", codec_case("table-sd-dec-B2-16x16-up-bf16x3", ("sd", True, (2, 4, 16, 16), "bf16x3", _UP, set())),
      [row("M256N64", 2, FL_ALL, 1)], 8192)


@pytest.mark.parametrize("cid", list(CASES))
def test_case_gates_its_rows(cid):
    led = run_case(cid)
    print(f"\n[{cid}] {led['kind']}: " + ", ".join(f"{k} {v:.2e}" if isinstance(v, float) else f"{k} {v}" for k, v in led["worst"].items()))
    for r in sorted(led["rows"]):
        print(f"    {describe(r)}")
    assert CASES[cid][2] <= led["rows"]


def test_every_row_is_gated_or_provably_unselectable():
    for cid in CASES:
        if cid not in LEDGER:                       # (this test run on its own)
            run_case(cid)
    tab = table()
    n_direct = {r for r, c in GATED.items() if any(LEDGER[x.split("+")[0]]["kind"] == "direct" for x in c) and not stamped(r)}
    n_plan = {r for r, c in GATED.items() if any(LEDGER[x.split("+")[0]]["kind"] == "plan" for x in c) and not stamped(r)}
    n_stamp = {r for r in GATED if stamped(r)}
    print(f"\n{len(tab)} rows: {len(GATED)} gated ({len(n_direct)} directly, {len(n_plan)} through plans, {len(n_stamp)} as stamped twins), {len(ALLOW)} allowed")
    for cid, led in LEDGER.items():
        print(f"[{cid}] {len(led['rows'])} rows; " + ", ".join(f"{k} {v:.2e}" if isinstance(v, float) else f"{k} {v}" for k, v in led["worst"].items()))
    missing = tab - set(GATED) - set(ALLOW)
    assert len(ALLOW) <= 20
    assert ROUTES <= tab, f"route lines that are no row of the table: {sorted(ROUTES - tab)}"
    assert not (set(GATED) & set(ALLOW)), f"allowed rows that a case launched (stale allow-list): {[describe(r) for r in sorted(set(GATED) & set(ALLOW))]}"
    assert not missing, f"{len(missing)} rows without a case:\n" + "\n".join("    " + describe(r) for r in sorted(missing))
    assert tab == set(GATED) | set(ALLOW)
