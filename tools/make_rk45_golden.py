#!/usr/bin/env python3
"""tests/golden/rk45_scipy_oracle.npz: the legacy adaptive sampler (legacy/train_sd_flowers.py:78-107, scipy.integrate.solve_ivp(method="RK45",
rtol = atol = 1e-5) over (1e-3, 1)) around the CPU oracle U-Net (oracle.flow_oracle.velocity_cfg), for the GPU tests of the library's RK45
(tests/test_gpu_rk45.py).  Each case stores its source, class ids, final latents and scipy's nfev / accepted / rejected counts; the weights
are rebuilt from the seed by `rk45_case_weights` (a fresh Unet's default init, 1-D parameters + 0.1 randn) or `oracle.synth`.

    python tools/make_rk45_golden.py        (several minutes on the host: hundreds of oracle forwards per case)
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import flow_oracle as fo  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "rk45_scipy_oracle.npz")
EPS, RTOL, ATOL = 1e-3, 1e-5, 1e-5

# name: (model kwargs or "d8mask", weight seed, batch, HxW, class ids, cfg, source seed)
CASES = {
    "d16_cfg0": (dict(dim=16, n_classes=10), 5, 2, 16, [5, 8], 0.0, 105),
    "d16_cfg3": (dict(dim=16, n_classes=10), 5, 2, 16, [5, 8], 3.0, 105),
    "d16_other": (dict(dim=16, n_classes=10), 5, 2, 16, [1, 9], 0.0, 205),
    "d8mask": ("d8mask", 3, 2, 8, None, 3.0, 3),
    "d32": (dict(dim=32, n_classes=102), 7, 3, 32, [7, 50, 101], 0.0, 107),
}


def rk45_case_weights(kw, seed):
    """State dict of a case: torch.manual_seed(seed); Unet(...) default init; every 1-D parameter + 0.1 randn (so every parameter matters)."""
    from flocoder_amd.unet import Unet
    torch.manual_seed(seed)
    m = Unet(dim_mults=(1, 2, 4, 8), channels=4, **kw).eval()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(seed)
    for k, v in sd.items():
        if v.dtype == torch.float32 and v.ndim == 1:
            sd[k] = v + 0.1 * torch.randn(v.shape, generator=g)
    return sd


def d8mask_weights(seed):
    from oracle.synth import synth_state_dict
    with np.load(os.path.join(ROOT, "tests", "golden", "g3_unet_d8mask.npz")) as z:
        shapes = json.loads(str(z["shapes"]))
        mask = torch.from_numpy(z["mask"])
    return synth_state_dict(shapes, seed), mask


@torch.no_grad()
def scipy_oracle(sd, z0, cond, cfg):
    """(latents, nfev, accepted, rejected) of solve_ivp(RK45) on velocity_cfg, as the legacy sampler drives its model."""
    from scipy.integrate import solve_ivp
    shape = tuple(z0.shape)

    def f(t, y):
        x = torch.from_numpy(y.reshape(shape)).type(torch.float32)
        return fo.velocity_cfg(sd, cond, cfg, x, t).numpy().reshape(-1)

    sol = solve_ivp(f, (EPS, 1), z0.numpy().reshape(-1), method="RK45", rtol=RTOL, atol=ATOL)
    assert sol.success, sol.message
    acc = len(sol.t) - 1
    return torch.tensor(sol.y[:, -1]).reshape(shape).type(torch.float32), int(sol.nfev), acc, (int(sol.nfev) - 2) // 6 - acc


def case_inputs(name):
    kw, seed, b, hw, ids, cfg, src_seed = CASES[name]
    z0 = torch.randn(b, 4, hw, hw, generator=torch.Generator().manual_seed(src_seed))
    if kw == "d8mask":
        sd, mask = d8mask_weights(seed)
        return sd, z0, {"class_cond": None, "mask_cond": mask}, cfg
    return rk45_case_weights(kw, seed), z0, {"class_cond": torch.tensor(ids)}, cfg


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    names = sys.argv[1:] or list(CASES)
    out = dict(np.load(OUT)) if os.path.exists(OUT) else {}
    for name in names:
        sd, z0, cond, cfg = case_inputs(name)
        lat, nfev, acc, rej = scipy_oracle(sd, z0, cond, cfg)
        out[f"{name}.source"] = z0.numpy()
        out[f"{name}.latents"] = lat.numpy()
        out[f"{name}.counts"] = np.array([nfev, acc, rej], dtype=np.int64)
        print(json.dumps({"case": name, "nfev": nfev, "accepted": acc, "rejected": rej}), flush=True)
    np.savez_compressed(OUT, **out)


if __name__ == "__main__":
    main()
