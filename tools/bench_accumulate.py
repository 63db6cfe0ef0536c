#!/usr/bin/env python3
"""What gradient accumulation costs at the stl_sd.yaml shape (batch 64, latents 4x32x32, U-Net dim 32, 10 classes): time per optimiser
step of ``FlowTrainer.step`` for micro_batch in {None, 32, 16}, and a step over 256 rows in micro-batches of 64 against four plain
steps of 64.

The expectation checked: an accumulated step of K chunks costs no more than K plain steps' forward + backward plus ONE optimiser tail,

    T_acc(K x b)  <=  K * (T_plain(b) - T_tail) + T_tail + margin,

with T_plain(b) the plain step at the chunk's batch (its own model, so the plan is the one the chunks run), T_tail the clip + Adam + EMA
+ weight re-upload timed alone, and the margin K times the run-to-run spread (max - min over the repeats) of T_plain(b) measured here:
the plain step is the code path every earlier version of the library runs, bit for bit, so that spread is what two runs of the same
code differ by on this machine.  Each figure is the median over ``--repeats`` windows of ``--steps`` steps, the windows of all
configurations interleaved; a window is a host clock around steps that end in a device synchronise.

    python tools/bench_accumulate.py [--steps K --warmup W --repeats R --out profiles/accumulate_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIM, HW, NCLS = 32, 32, 10


class Leg:
    """One configuration: its own model and trainer (the launch plan is built for the rows it reserves), fixed synthetic inputs."""

    def __init__(self, device, rows, micro_batch, plain_steps=1):
        from flocoder_amd.train import FlowTrainer
        from flocoder_amd.unet import Unet
        torch.manual_seed(0)
        self.tr = FlowTrainer(Unet(dim=DIM, dim_mults=(1, 2, 4, 8), channels=4, n_classes=NCLS).to(device), lr=1e-4, distributed=False)
        g = torch.Generator().manual_seed(99)
        self.src = torch.randn(rows, 4, HW, HW, generator=g).to(device)
        self.tgt = torch.randn(rows, 4, HW, HW, generator=g).to(device)
        self.cond = {"class_cond": torch.randint(NCLS, (rows,), generator=g).to(device), "mask_cond": None}
        self.micro_batch, self.plain_steps, self.device, self.times = micro_batch, plain_steps, device, []

    def one(self):
        if self.plain_steps > 1:                     # the same rows as consecutive plain steps: K optimiser steps instead of one
            b = self.src.shape[0] // self.plain_steps
            for k in range(self.plain_steps):
                rows = slice(k * b, (k + 1) * b)
                loss = self.tr.step(self.src[rows], self.tgt[rows], {"class_cond": self.cond["class_cond"][rows], "mask_cond": None})
            return loss
        return self.tr.step(self.src, self.tgt, self.cond, micro_batch=self.micro_batch)

    def tail(self):
        self.tr.optimizer_step(has_class_grads=True)

    def window(self, fn, steps):
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize(self.device)
        return 1e3 * (time.perf_counter() - t0) / steps


def summary(ms):
    return {"ms": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "spread": round(max(ms) - min(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accumulate_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_accumulate needs an MI355X: there is nothing to time without one")
    device = torch.device("cuda", 0)
    legs = {
        "plain_64": Leg(device, 64, None),
        "plain_32": Leg(device, 32, None),
        "plain_16": Leg(device, 16, None),
        "acc_64_as_2x32": Leg(device, 64, 32),
        "acc_64_as_4x16": Leg(device, 64, 16),
        "acc_256_as_4x64": Leg(device, 256, 64),
        "four_plain_steps_of_64": Leg(device, 256, None, plain_steps=4),
    }
    tails = {k: [] for k in ("plain_64", "plain_32", "plain_16")}
    for leg in legs.values():
        for _ in range(args.warmup):
            loss = leg.one()
        assert torch.isfinite(loss)
    for _ in range(args.repeats):                    # interleaved: every configuration sees the same weather
        for name, leg in legs.items():
            leg.times.append(leg.window(leg.one, args.steps))
            if name in tails:
                tails[name].append(leg.window(leg.tail, args.steps))
    res = {name: summary(leg.times) for name, leg in legs.items()}
    tail = {name: summary(v) for name, v in tails.items()}
    checks = []
    for acc, plain, k in (("acc_64_as_2x32", "plain_32", 2), ("acc_64_as_4x16", "plain_16", 4), ("acc_256_as_4x64", "plain_64", 4)):
        bound = k * (res[plain]["ms"] - tail[plain]["ms"]) + tail[plain]["ms"]
        margin = k * res[plain]["spread"]
        checks.append({"accumulated": acc, "chunks": k, "chunk_step": plain, "ms": res[acc]["ms"], "bound_ms": round(bound, 4),
                       "margin_ms": round(margin, 4), "verdict": "met" if res[acc]["ms"] <= bound + margin else "missed"})
    out = {"workload": f"FlowTrainer.step, U-Net dim={DIM} dim_mults [1,2,4,8] n_classes={NCLS}, latents 4x{HW}x{HW}, fixed synthetic inputs, no pairing; "
                       f"median of {args.repeats} interleaved windows of {args.steps} steps, one GPU",
           "device": torch.cuda.get_device_name(0), "ms_per_optimizer_step": res, "optimizer_tail_ms": tail,
           "ms_per_256_rows": {"acc_256_as_4x64": res["acc_256_as_4x64"]["ms"], "four_plain_steps_of_64": res["four_plain_steps_of_64"]["ms"]},
           "expectation": "T_acc(K x b) <= K (T_plain(b) - T_tail) + T_tail + K spread(T_plain(b))", "checks": checks}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
