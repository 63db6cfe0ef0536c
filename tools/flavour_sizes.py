#!/usr/bin/env python3
"""Code size of the pipelined convolution's instantiations (`conv_pipe_kernel<...>`), from the SYMBOL TABLE of the gfx950 code objects
inside the built library: symbol sizes only (llvm-readelf -s), nothing is disassembled.

    python tools/flavour_sizes.py [--lib PATH] [--plan [--sizes-of PATH]]

Without --plan (no GPU needed): every instantiation and its .text bytes.  With --plan (needs the GPU): one eager forward of the bench
model with the route record on (fc_debug_conv_routes), then only the instantiations that forward launched, each with the plan entries
that use it.  The instruction cache is cold at every launch, so a Block-closing flavour's bytes are paid per launch.
"""
import argparse
import ctypes as C
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
READELF = os.environ.get("LLVM_READELF", "/opt/rocm/lib/llvm/bin/llvm-readelf")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
ARGS = ("WM", "WN", "WK", "MT", "NT", "CC", "NPL", "KS", "NL", "FL", "PREC", "GEO", "GEO1")    # GEO: key of a Block-closing flavour, GEO1: of a conv1 flavour
FL_NAMES = {1: "fin", 2: "res", 4: "post", 8: "xf", 16: "cat", 32: "stamp", 64: "stats", 128: "gn1", 256: "postop", 512: "narrow", 1024: "multi",
            2048: "meet", 4096: "w4", 8192: "ww", 16384: "step"}


def code_objects(path):
    """The gfx950 ELF images of every offload bundle in the library."""
    blob = open(path, "rb").read()
    for m in re.finditer(MAGIC, blob):
        p = m.start()
        (n,) = struct.unpack_from("<Q", blob, p + len(MAGIC))
        o = p + len(MAGIC) + 8
        for _ in range(n):
            off, size, idlen = struct.unpack_from("<QQQ", blob, o)
            o += 24
            ident = blob[o:o + idlen].decode()
            o += idlen
            if "gfx950" in ident and size:
                yield blob[p + off:p + off + size]


def kernel_sizes(path):
    """{(thirteen template arguments): .text bytes} of every conv_pipe_kernel instantiation."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, img in enumerate(code_objects(path)):
            f = os.path.join(tmp, f"co{i}.elf")
            open(f, "wb").write(img)
            txt = subprocess.run([READELF, "-s", "-W", "--demangle", f], capture_output=True, text=True, check=True).stdout
            for line in txt.splitlines():
                m = re.match(r"\s*\d+:\s+[0-9a-f]+\s+(\d+)\s+FUNC\s+.*\bconv_pipe_kernel<([^>]*)>", line)
                if m:
                    a = [int(x) for x in m.group(2).split(",")]
                    a += [0] * (len(ARGS) - len(a))                              # (a build from before the geometry keys has eleven or twelve)
                    out[tuple(a)] = int(m.group(1))
    return out


def describe(key):
    d = dict(zip(ARGS, key))
    tile = f"M{32 * d['MT'] * d['WM']}N{32 * d['NT'] * d['WN']}" + (f"K{d['WK']}" if d["WK"] > 1 else "")
    fl = "all-in-one" if d["FL"] == 4095 else ("+".join(n for b, n in FL_NAMES.items() if d["FL"] & b) or "plain")
    geo = ""
    if d["GEO"] or d["GEO1"]:
        g = d["GEO"] or d["GEO1"]
        geo = f" geo[{('?', 'pair', 'fast', 'general')[g & 3]} TB{1 + ((g >> 2) & 1)} TW{1 << ((g >> 3) & 7)} cpg{1 << ((g >> 6) & 15)} Tst{(g >> 10) & 63}]"
    return f"{tile} {d['KS']}x{d['KS']}{' bf16x3' if d['PREC'] else ''} {fl}{geo}"


def plan_routes():
    """[(module, plan kernel name, template arguments)] of the convolutions of one forward of the bench model."""
    import torch
    import bench
    from flocoder_amd import _binding as B
    lib = B.lib()
    dev = torch.device("cuda:0")
    model = bench.build_model(dev)
    model.reserve(bench.BATCH, 32, 32, dev)
    rows = model.profile_ops(bench.BATCH, repeats=1)                # (also leaves finite data in the plan's buffers)
    B.check(lib.fc_debug_conv_routes(1))
    model.profile_ops(bench.BATCH, repeats=1)
    torch.cuda.synchronize()
    B.check(lib.fc_debug_conv_routes(0))
    n = lib.fc_debug_conv_routes_read(None, 0)
    buf = C.create_string_buffer(n + 1)
    lib.fc_debug_conv_routes_read(buf, n + 1)
    routes = [tuple(int(x) for x in l.split()) for l in buf.value.decode().splitlines()]
    convs = [r for r in rows if r["kernel"].startswith("conv_igemm")]
    # profile_ops runs the plan once (warm) and then every entry `repeats` times, in plan order: the last len(convs) launches are the entries
    if not convs or len(routes) != 2 * len(convs):
        raise SystemExit(f"route record does not line up with the plan: {len(routes)} launches, {len(convs)} convolution entries")
    return [(c["module"], c["kernel"], r) for c, r in zip(convs, routes[len(convs):])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.environ.get("FLOCODER_AMD_LIB") or os.path.join(ROOT, "flocoder_amd", "_lib", "libflocoder_amd.so"))
    ap.add_argument("--plan", action="store_true", help="only the flavours the dim-32 inference plan launches, with the plan entries (GPU)")
    ap.add_argument("--sizes-of", metavar="PATH", help="with --plan: look the sizes up in another build of the library; a launch whose (mask, geometry) "
                    "flavour that build does not have is listed with its flavour of the same mask and run-time geometry")
    a = ap.parse_args()
    sizes = kernel_sizes(a.sizes_of or a.lib)
    print(f"# {os.path.basename(a.sizes_of or a.lib)}: {len(sizes)} conv_pipe_kernel instantiations, {sum(sizes.values())} bytes of .text")
    if not a.plan:
        for k, v in sorted(sizes.items(), key=lambda kv: (describe(kv[0]), kv[1])):
            print(f"{describe(k):70s} {v:7d}")
        return
    os.environ["FLOCODER_AMD_LIB"] = a.lib
    users = {}
    for module, kernel, key in plan_routes():
        key = tuple(key) + (0,) * (len(ARGS) - len(key))
        if key not in sizes and key[:11] + (0, 0) in sizes:
            key = key[:11] + (0, 0)
        users.setdefault(key, []).append(module + ("+fin" if kernel.endswith("+fin") else ""))
    for k, mods in sorted(users.items(), key=lambda kv: describe(kv[0])):
        print(f"{describe(k):70s} {sizes.get(k, -1):7d}   {' '.join(mods)}")


if __name__ == "__main__":
    main()
