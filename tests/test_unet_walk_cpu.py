"""walk_unet (csrc/unet_walk.h) keeps the liveness protocol and unet.py's module order: tests/unet_walk_check.cpp drives it with a
recording emitter over one to four levels, with and without mask conditioning, and checks that every tensor an emitter call reads is
still alive, that every tensor is retired at most once and everything but the output exactly once by the time the walk returns (so
nothing is left on the skip stack), that skips are consumed in the reverse of the order unet.py appends them, and the module sequence
of the four-level mask model.  Host code only: built with the host compiler under AddressSanitizer and UBSan, run as a program of its own.
"""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "flocoder_amd", "csrc")


def test_walk_protocol_and_module_order(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "unet_walk_check")
    build = subprocess.run([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                            os.path.join(HERE, "unet_walk_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
