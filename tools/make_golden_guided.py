#!/usr/bin/env python3
"""Generate tests/golden/g12_algorithm3.npz by running the *reference's* ``algorithm3`` (flocoder/inpainting.py:92-130) in fp64.

Run in the build container only (``python tools/make_golden_guided.py``), like tools/make_golden.py: the reference's file is imported
from FLOCODER_REFERENCE, never copied; only inputs and outputs (a few KB of data) are written.  Cases, one flattened sample each:
a selection-row ``A`` built from a 0/1 mask and a random dense ``A``; tp in {0.1, 0.5, 0.9}; sigma_y in {0.05, 0.5}; gamma in {1, 0.5}.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from make_golden import REF  # noqa: E402  (where the reference lies: FLOCODER_REFERENCE)
from oracle.synth import synth_input  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "g12_algorithm3.npz")
SHAPE = (1, 4, 4, 4)          # n = 64 unknowns
K_DENSE = 24


def import_reference_inpainting():
    for name in ("PIL", "PIL.Image"):
        try:
            importlib.import_module(name)
        except Exception:                      # absent third-party module the function under test never touches
            sys.modules[name] = types.ModuleType(name)
    if not hasattr(sys.modules["PIL"], "Image"):
        sys.modules["PIL"].Image = sys.modules["PIL.Image"]
    spec = importlib.util.spec_from_file_location("ref_inpainting", os.path.join(REF, "flocoder", "inpainting.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = import_reference_inpainting()
    torch.set_default_dtype(torch.float64)      # the function builds its identity matrix in the default dtype
    n =int(np.prod(SHAPE))
    v = synth_input("g12.v", SHAPE, 12).double()
    x = synth_input("g12.x", SHAPE, 12).double()
    known = synth_input("g12.known", SHAPE, 12).double()
    mask = (synth_input("g12.mask", SHAPE, 12) > 0.1).double().flatten()        # 1 = measured
    rows = torch.nonzero(mask).flatten()
    a_sel = torch.zeros(len(rows), n, dtype=torch.float64)
    a_sel[torch.arange(len(rows)), rows] = 1.0
    a_dense = synth_input("g12.A", (K_DENSE, n), 12).double() / np.sqrt(n)
    arrays = dict(v=v, x=x, known=known, mask=mask.reshape(SHAPE), A_selection=a_sel, A_dense=a_dense)
    cases = []
    for kind, A in (("selection", a_sel), ("dense", a_dense)):
        y = A @ known.flatten()
        arrays[f"y_{kind}"] = y
        for tp in (0.1, 0.5, 0.9):
            for sigma_y in (0.05, 0.5):
                for gamma in (1.0, 0.5):
                    out = ref.algorithm3(v, x, 0.0, tp, y, A, sigma_y=sigma_y, gamma_t=gamma)
                    assert out.dtype == torch.float64 and bool(torch.isfinite(out).all())
                    arrays[f"out_{len(cases)}"] = out
                    cases.append((kind, tp, sigma_y, gamma))
    arrays["case_kind"] = np.array([c[0] for c in cases])
    arrays["case_tp"] = np.array([c[1] for c in cases], dtype=np.float64)
    arrays["case_sigma_y"] = np.array([c[2] for c in cases], dtype=np.float64)
    arrays["case_gamma"] = np.array([c[3] for c in cases], dtype=np.float64)
    conv = {k: (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t) for k, t in arrays.items()}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **conv)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KiB, {len(cases)} cases)")


if __name__ == "__main__":
    main()
