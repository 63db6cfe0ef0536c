#!/usr/bin/env python3
"""tests/golden/rk45_per_sample_scipy_oracle.npz: per-sample adaptive RK45, the contract of fc_unet_integrate_rk45_per_sample
(tests/test_gpu_rk45_per_sample.py).  Every sample b of a case is its OWN scipy.integrate.solve_ivp(method="RK45", rtol = atol = 1e-5)
problem over (1e-3, 1): its C*H*W unknowns alone, f_b = the CPU oracle U-Net (oracle.flow_oracle.velocity_cfg) on that one sample with
its class id and mask row.  The cases, weights and sources are tools/make_rk45_golden.py's (imported, not restated), plus "d16_mixed",
whose samples start at different scales so that their step sequences differ.  Each case stores its source, the per-sample latents and
per-sample [nfev, accepted, rejected] ([B, 3]).

    python tools/make_rk45_per_sample_golden.py        (minutes on the host: hundreds of oracle forwards per sample)
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.make_rk45_golden import CASES, case_inputs, rk45_case_weights, scipy_oracle  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "rk45_per_sample_scipy_oracle.npz")

SHARED = ("d16_cfg0", "d16_cfg3", "d8mask", "d32")
# d16_mixed: the d16 model (weight seed 5), class ids [5, 8, 2], no guidance; randn(seed 305) with sample b scaled by MIXED_SCALES[b]
MIXED_SCALES = (1.0, 0.05, 4.0)


def per_sample_inputs(name):
    """(state dict, source [B,C,H,W], cond, cfg) of a case."""
    if name == "d16_mixed":
        kw, seed = CASES["d16_cfg0"][0], CASES["d16_cfg0"][1]
        z0 = torch.randn(len(MIXED_SCALES), 4, 16, 16, generator=torch.Generator().manual_seed(305))
        z0 = z0 * torch.tensor(MIXED_SCALES).view(-1, 1, 1, 1)
        return rk45_case_weights(kw, seed), z0, {"class_cond": torch.tensor([5, 8, 2])}, 0.0
    return case_inputs(name)


def sample_cond(cond, b):
    return {k: (v[b:b + 1] if v is not None else None) for k, v in cond.items()}


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    names = sys.argv[1:] or list(SHARED) + ["d16_mixed"]
    out = dict(np.load(OUT)) if os.path.exists(OUT) else {}
    for name in names:
        sd, z0, cond, cfg = per_sample_inputs(name)
        lats, counts = [], []
        for b in range(z0.shape[0]):
            lat, nfev, acc, rej = scipy_oracle(sd, z0[b:b + 1], sample_cond(cond, b), cfg)
            lats.append(lat)
            counts.append([nfev, acc, rej])
        out[f"{name}.source"] = z0.numpy()
        out[f"{name}.latents"] = torch.cat(lats).numpy()
        out[f"{name}.counts"] = np.array(counts, dtype=np.int64)
        print(json.dumps({"case": name, "counts": counts}), flush=True)
    np.savez_compressed(OUT, **out)


if __name__ == "__main__":
    main()
