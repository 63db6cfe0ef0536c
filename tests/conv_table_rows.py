"""Names for the rows of the pipelined convolution's instantiation table, and the ledger's allow-list (test helper, imported by
tests/test_conv_table_cpu.py and tests/test_gpu_conv_table.py; not a conftest).

A row is the tuple of the thirteen template arguments of one conv_pipe_kernel instantiation, as fc_debug_conv_routes_read and
fc_debug_conv_table_read print them: WM WN WK MT NT CC NPL KS NL FL PREC GEOF GEOK1 (conv_pipe.hip PipeRow::targ).
"""
A_KS, A_FL, A_PREC, A_GEOF, A_GEO1 = 7, 9, 10, 11, 12
FL_FIN, FL_RES, FL_POST, FL_XF, FL_CAT, FL_STAMP, FL_STATS, FL_GN1, FL_POSTOP = 1, 2, 4, 8, 16, 32, 64, 128, 256
FL_NARROW, FL_MULTI, FL_MEET, FL_ALL, FL_W4, FL_WW, FL_STEP = 512, 1024, 2048, 4095, 4096, 8192, 16384
FL_NAMES = {FL_FIN: "fin", FL_RES: "res", FL_POST: "post", FL_XF: "xf", FL_CAT: "cat", FL_STAMP: "stamp", FL_STATS: "stats", FL_GN1: "gn1",
            FL_POSTOP: "postop", FL_NARROW: "narrow", FL_MULTI: "multi", FL_MEET: "meet", FL_W4: "w4", FL_WW: "ww", FL_STEP: "step"}
# conv_dev.h kConvTiles: WM WN WK MT NT CC, and the staging waves at kernel sizes above 1x1
TILES = {"M128N32": (4, 1, 1, 1, 1, 16, 4), "M128N64": (4, 1, 1, 1, 2, 16, 4), "M64N32K2": (2, 1, 2, 1, 1, 32, 8),
         "M32N32K4": (1, 1, 4, 1, 1, 32, 8), "M64N64K2": (2, 1, 2, 1, 2, 16, 4), "M256N64": (4, 1, 1, 2, 2, 16, 4)}
LEAN_TILES = ("M32N32K4", "M64N32K2", "M128N32")
BF3_TILES = ("M128N32", "M128N64", "M256N64")
BM = {t: 32 * v[3] * v[0] for t, v in TILES.items()}
BN = {t: 32 * v[4] * v[1] for t, v in TILES.items()}


def row(tile, ks, fl, prec=0, geof=0, geo1=0):
    """The row of (tile, kernel size, mask, precision, keys) as conv_pipe.hip add_row() names it."""
    t = TILES[tile]
    return (*t[:6], 8 if fl == FL_ALL else 4, ks, 4 if ks == 1 else t[6], fl, prec, geof, geo1)


def geo_key(form, TB, TW, cpg, Tst):
    """conv_dev.h geo_key: form 1 pair / 2 fast."""
    lg = lambda v: v.bit_length() - 1
    return form | ((1 if TB == 2 else 0) << 2) | (lg(TW) << 3) | (lg(cpg) << 6) | (Tst << 10)


def tile_of(r):
    return next(t for t, v in TILES.items() if tuple(r[:6]) == v[:6])


def lean(r):
    return r[A_FL] != FL_ALL


def stamped(r):
    return lean(r) and bool(r[A_FL] & FL_STAMP)


def with_fl(r, fl):
    return tuple(r[:A_FL]) + (fl,) + tuple(r[A_FL + 1:])


def all_in_one(r):
    """The all-in-one row of r's tile and kernel size (exact fp32)."""
    return row(tile_of(r), r[A_KS], FL_ALL)


def describe(r):
    fl = "all-in-one" if r[A_FL] == FL_ALL else ("+".join(n for b, n in FL_NAMES.items() if r[A_FL] & b) or "plain")
    key = (f" geof={r[A_GEOF]}" if r[A_GEOF] else "") + (f" geo1={r[A_GEO1]}" if r[A_GEO1] else "")
    return f"{tile_of(r)} {r[A_KS]}x{r[A_KS]}{' bf16x3' if r[A_PREC] else ''} {fl}{key}"


# Rows NO caller can select, each with the condition that shows it.  Not "hard to reach": a row that some shape, batch or plan form
# selects belongs in a case of tests/test_gpu_conv_table.py.  At most 20 (a tenth of the table); the closing test of the ledger fails when
# a row listed here is launched by any case (a stale entry), tests/test_conv_table_cpu.py when one is no row of the table any more.
_RES_NO_CAT = ("FL_STATS|FL_RES without FL_CAT: pipe_need() sets FL_RES only for ConvArgs::res_out, which the one planner that fuses a res_conv "
               "(unet.hip Builder::resblock, cin != cout) sets together with the concatenated skip -- every Block of the U-Net whose input and "
               "output widths differ is an up-path Block or final_res_block, all built with `skip` -- and fc_debug_conv has no res output")
_XF_STATS_1 = ("1x1 FL_STATS|FL_XF: no planner builds a 1x1 convolution with both a transform loader and output statistics -- unet.hip to_qkv "
               "has the loader and conv(a, qkv, 0, nullptr), to_out has statistics and an untransformed source; vqvae.hip's 1x1 launches with "
               "b.gn(...) sources (attn.qkv, decoder L+3) pass groups 0, those with groups (encoder 2nd+2, decoder L, downsample.0) no xf; vae.hip's "
               "1x1 launches have neither -- and fc_debug_conv has no transform loader, so pipe_need() never yields this mask at KS = 1")
_KS5_LDS = ("5x5 on this tile: conv_igemm.hip conv_geometry(pipe) carves two weight stages of KS*KS*CC*BN floats (wl_stride, nwb >= 2) = "
            "2 x 25 x {cc} x {bn} x 4 B = {kb} KiB, above the 160 KiB it then tests (\"tile does not fit in LDS\"), for every shape: "
            "geometry_best() falls to the synchronous kernel (M256N64: refuses), so conv_pipe_select() is never asked for this row")
ALLOW = {
    **{row(t, 3, FL_STATS | FL_RES): _RES_NO_CAT for t in LEAN_TILES},
    row("M32N32K4", 3, FL_STATS | FL_RES | FL_W4): _RES_NO_CAT,
    **{row(t, 1, FL_STATS | FL_XF): _XF_STATS_1 for t in LEAN_TILES + ("M256N64", "M128N64")},
    **{row(t, 5, FL_ALL): _KS5_LDS.format(cc=TILES[t][5], bn=BN[t], kb=2 * 25 * TILES[t][5] * BN[t] * 4 // 1024)
       for t in ("M128N64", "M64N32K2", "M32N32K4", "M64N64K2", "M256N64")},
}
