#!/usr/bin/env python3
"""Flow log-likelihood at the headline's model and batch: flowers-sized U-Net (dim 32, dim_mults [1,2,4,8], 102 classes, weights seeded as
bench.py seeds them), B=64 latents of 4x32x32, class ids, n_steps grid points.  Prints ONE JSON line (profiles/likelihood_bench.json):

  ll_ms_per_eval           wall time of a whole sampling.log_likelihood call over its 4 (n_steps - 1) evaluations (median of --reps calls;
                           an evaluation is a training-mode forward, the backward plan's data-gradient chain and one stage kernel), on a
                           model whose plans are in the training form already (no plan is rebuilt inside the timed call)
  ll_ms_per_call_from_inference_form   the same call on a model that samples: it switches the plans to the training form and back
                           (a device synchronisation and two plan builds inside the call)
  rk4_ms_per_eval          sampling.generate_latents_rk4 (no guidance) on the same model, batch and grid size over ITS 4 (n_steps - 1)
                           evaluations, alternating with the likelihood calls in this process: the yardstick
  invert_ms_per_eval       sampling.invert_latents (the same captured path on the reversed grid), alternating as well
  vjp_x_ms / backward_ms   Unet.vjp_x against the full Unet.backward_native(want_dx=True) for the same training forward, alternating,
                           each timed over --inner back-to-back calls between device synchronisations; vjp_speedup = their ratio.
                           vjp_x slower than the full backward fails the tool: it runs a strict subset of its launches.
  launches_per_eval        forward plan + data-gradient mode + the stage kernel

    python tools/bench_likelihood.py [--reps 5] [--n-steps 50] [--inner 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if not os.environ.get("FLOCODER_AMD_KEEP_ENV"):
    os.environ.setdefault("AMD_DIRECT_DISPATCH", "0")      # the sampler's shipping runtime mode, as bench.py

import torch  # noqa: E402

BATCH, LATENT, DIM, NCLS = 64, (4, 32, 32), 32, 102


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-steps", type=int, default=50)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    from flocoder_amd import _binding as B
    from flocoder_amd import sampling as S
    from flocoder_amd.metrics import bits_per_dim
    from flocoder_amd.unet import Unet
    if not torch.cuda.is_available():
        sys.exit("bench_likelihood needs an MI355X")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    shape = (BATCH,) + LATENT
    ids = torch.randint(NCLS, (BATCH,), generator=torch.Generator().manual_seed(1235)).to(dev)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1234)).to(dev)
    eps = (torch.randint(0, 2, shape, generator=torch.Generator().manual_seed(1236)).float() * 2 - 1).to(dev)
    cond = {"class_cond": ids}
    # two models with the same weights: `model` is put into the training form of its plans once, so that the timed likelihood calls
    # rebuild nothing; `sampler_model` stays a model that samples (inference-form plans): the yardstick, and the "from inference form" call
    model = Unet(dim=DIM, dim_mults=(1, 2, 4, 8), channels=LATENT[0], n_classes=NCLS).eval().to(dev)
    sampler_model = model.replica()
    model._forward_native(x, torch.full((BATCH,), 500.0, device=dev), ids, None, train=True)
    evals = 4 * (a.n_steps - 1)

    def ll():
        return S.log_likelihood(model, x, n_steps=a.n_steps, cond=cond, probe=eps)

    def rk4():
        return S.generate_latents_rk4(sampler_model, shape, a.n_steps, cond, 0.0, source=x)

    def inv():
        return S.invert_latents(sampler_model, x, n_steps=a.n_steps, cond=cond)

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out

    (logp, z, nfe), _, _ = ll(), rk4(), inv()                # warm: plans, graphs, code objects
    assert nfe == evals and torch.isfinite(logp).all()
    t_ll, t_rk4, t_inv = [], [], []
    for _ in range(a.reps):
        t_ll.append(timed(ll)[0])
        t_rk4.append(timed(rk4)[0])
        t_inv.append(timed(inv)[0])
    t_cold = [timed(lambda: S.log_likelihood(sampler_model, x, n_steps=a.n_steps, cond=cond, probe=eps))[0] for _ in range(max(2, a.reps // 2))]
    zi = inv()[0]
    zrel = float(((z.double() - zi.double()).flatten(1).norm(dim=1) / zi.double().flatten(1).norm(dim=1)).max())

    # the data-gradient chain alone against the full backward, for one training forward
    tvec = torch.full((BATCH,), 500.0, device=dev)
    model._forward_native(x, tvec, ids, None, train=True)
    flat = torch.empty(model._flat_numel, dtype=torch.float32, device=dev)
    dx_full = model.backward_native(x, tvec, ids, eps, grads=flat, want_dx=True)[1].clone()
    dx_only = model.vjp_x(x, tvec, ids, eps)
    assert torch.equal(dx_full, dx_only), "vjp_x and the full backward disagree on d(x)"
    dxbuf = torch.empty_like(x)

    def full_backward():
        for _ in range(a.inner):
            model.backward_native(x, tvec, ids, eps, grads=flat, want_dx=True, dx=dxbuf)

    def only_dx():
        for _ in range(a.inner):
            model.vjp_x(x, tvec, ids, eps)

    full_backward(); only_dx()
    t_b, t_v = [], []
    for _ in range(a.reps):
        t_b.append(timed(full_backward)[0] / a.inner)
        t_v.append(timed(only_dx)[0] / a.inner)
    lib = B.lib()
    fwd_l, vjp_l, bwd_l = lib.fc_unet_plan_launches(model._handle), lib.fc_unet_vjp_launches(model._handle), lib.fc_unet_backward_launches(model._handle)
    ms = lambda v: statistics.median(v) * 1e3
    rec = {"tool": "bench_likelihood", "device": torch.cuda.get_device_name(dev), "batch": BATCH, "latent": list(LATENT), "dim": DIM,
           "n_classes": NCLS, "n_steps": a.n_steps, "evaluations": evals, "reps": a.reps,
           "AMD_DIRECT_DISPATCH": os.environ.get("AMD_DIRECT_DISPATCH"),
           "ll_ms_per_call": round(ms(t_ll), 2), "ll_ms_per_eval": round(ms(t_ll) / evals, 4),
           "ll_ms_per_call_from_inference_form": round(ms(t_cold), 2),
           "rk4_ms_per_eval": round(ms(t_rk4) / evals, 4), "invert_ms_per_eval": round(ms(t_inv) / evals, 4),
           "ll_over_rk4": round(ms(t_ll) / ms(t_rk4), 3),
           "ll_spread_ms": [round(min(t_ll) * 1e3, 2), round(max(t_ll) * 1e3, 2)],
           "rk4_spread_ms": [round(min(t_rk4) * 1e3, 2), round(max(t_rk4) * 1e3, 2)],
           "vjp_x_ms": round(ms(t_v), 4), "backward_ms": round(ms(t_b), 4), "vjp_speedup": round(ms(t_b) / ms(t_v), 3),
           "vjp_x_spread_ms": [round(min(t_v) * 1e3, 4), round(max(t_v) * 1e3, 4)],
           "backward_spread_ms": [round(min(t_b) * 1e3, 4), round(max(t_b) * 1e3, 4)],
           "forward_launches": fwd_l, "vjp_launches": vjp_l, "backward_launches": bwd_l, "launches_per_eval": fwd_l + vjp_l + 1,
           "mean_bits_per_dim": round(float(bits_per_dim(logp, x[0].numel()).mean()), 4),
           "z_vs_invert_rel_l2": zrel}
    print(json.dumps(rec), flush=True)
    if ms(t_v) > ms(t_b):
        sys.exit(f"vjp_x ({ms(t_v):.3f} ms) is slower than the full backward ({ms(t_b):.3f} ms): it runs a strict subset of its launches")


if __name__ == "__main__":
    main()
