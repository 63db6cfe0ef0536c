#!/usr/bin/env python3
"""Phase timeline of the Block-OPENING (conv1) convolution launches of the bench model's plan -- the first convolution of every ResnetBlock --
from the in-kernel stamps of ONE launch each (fc_debug_set_stamp_op, as tools/fin_stamps.py does for the Block-closing launches; the stamped
launch is the lean flavour the plan runs, plus the stamps, where the library has that flavour: the route column says which one ran).

    python tools/conv1_stamps.py [substring of the module name ...]        (default: all 19)

Columns, us since the tail-running wave's start (median over workgroups): first request (the staging waves' window / the accumulator waves'
weights), stage 0 ready, mfma done, statistics done, image written (LDS), last store issued; then `end`: first start -> last end of the
launch on the device-wide clock, and the launch's time in the op table.  `after mfma` = mfma done -> last store issued.
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from flocoder_amd import _binding as B  # noqa: E402

BLOCKS = ["downs.0.0", "downs.0.1", "downs.1.0", "downs.1.1", "downs.2.0", "downs.2.1", "downs.3.0", "downs.3.1", "mid_block1", "mid_block2",
          "ups.0.0", "ups.0.1", "ups.1.0", "ups.1.1", "ups.2.0", "ups.2.1", "ups.3.0", "ups.3.1", "final_res_block"]


def is_conv1(r):
    return r["module"] in BLOCKS and r["kernel"].startswith("conv_igemm") and not r["kernel"].endswith("+fin")


def stamped_route(lib):
    """The template arguments of the launch that ran with the stamps on: the one route of the record whose mask has the stamp bit (32) -- a lean
    stamped flavour, or, where the library has none for the mask, the all-in-one kernel (4095)."""
    n = lib.fc_debug_conv_routes_read(None, 0)
    buf = C.create_string_buffer(n + 1)
    lib.fc_debug_conv_routes_read(buf, n + 1)
    routes = [l.split() for l in buf.value.decode().splitlines()]
    lean = [r for r in routes if len(r) >= 12 and int(r[9]) & 32 and int(r[9]) != 4095]
    allin = [r for r in routes if len(r) >= 12 and int(r[9]) == 4095]
    return (lean or allin or [["?"] * 13])[-1]


def main():
    dev = torch.device("cuda:0")
    lib = B.lib()
    model = bench.build_model(dev)
    Bn = bench.BATCH
    model.reserve(Bn, 32, 32, dev)
    rows = model.profile_ops(Bn, repeats=3)
    want = sys.argv[1:]
    print(f"{'module':16s} {'kernel':24s} {'FL':>5s} {'GEO':>6s} {'wgs':>5s} | {'request':>7s} {'stage0':>7s} {'mfma':>7s} {'stats':>7s} {'image':>7s} {'stores':>7s} | "
          f"{'end':>7s} {'timed':>7s} | {'after mfma':>10s}")
    tot = 0.0
    for i, r in enumerate(rows):
        if not is_conv1(r) or (want and not any(w in r["module"] for w in want)):
            continue
        buf = torch.zeros(8192 * 8 * 16, dtype=torch.int64, device=dev)
        B.check(lib.fc_debug_set_stamp_op(i, buf.data_ptr()))
        B.check(lib.fc_debug_conv_routes(1))
        model.profile_ops(Bn, repeats=1)
        torch.cuda.synchronize()
        route = stamped_route(lib)
        B.check(lib.fc_debug_conv_routes(0))
        B.check(lib.fc_debug_set_stamp_op(-1, None))
        st = buf.view(8192, 8, 16).cpu()
        nb = int((st[:, 0, 0] != 0).sum())
        if nb == 0:
            print(f"{r['module']:16s} {r['kernel']:24s} no stamps (route {' '.join(route)})")
            continue
        st = st[:nb].double()
        ksplit = "K2" in r["kernel"] or "K4" in r["kernel"]
        cons = st[:, 0:1] if ksplit else st[:, 0:4]          # the waves that run the whole tail (wave 0 of a K-split tile)
        load = st[:, 4:8]
        t = lambda k: (cons[:, :, k] - cons[:, :, 0]).median().item() / 2.4e3
        req = min(t(1), (load[:, :, 1] - load[:, :, 0]).median().item() / 2.4e3)
        span = st[:, :, 8].max(dim=1).values - st[:, :, 0].min(dim=1).values
        rt = st[:, :, 15].min(dim=1).values * 10.0
        ends = rt + span / 2.4
        end = float(ends.max() - rt.min()) / 1e3
        fl, geo = route[9], route[-1]        # (the conv1 key is the last template argument)
        tot += t(8) - t(5)
        print(f"{r['module']:16s} {r['kernel']:24s} {fl:>5s} {geo:>6s} {nb:5d} | {req:7.2f} {t(4):7.2f} {t(5):7.2f} {t(14):7.2f} {t(9):7.2f} {t(8):7.2f} | "
              f"{end:7.2f} {1e3 * r['ms']:7.1f} | {t(8) - t(5):10.2f}")
    print(f"mfma done -> last store issued, summed over the listed launches: {tot:.2f} us")


if __name__ == "__main__":
    main()
