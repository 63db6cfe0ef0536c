#!/usr/bin/env python3
"""What an epoch's evaluation costs on the device: the note metrics and the codebook counting next to upstream's own lines in torch on
the same device, and evaluate_model next to the sum of its parts.

    python tools/bench_eval.py [--batches 64 256 --reps 10 --windows 5 --steps 10 --out profiles/eval_bench.json]

* calc_note_metrics at the midi_vqgan.yaml image shape (B x 3 x 128 x 128), with and without the images, against a torch restatement
  of upstream's loop (flocoder/metrics.py:362-455) on the same tensors; the fc_note_confusion launches alone between two device events,
  whose bytes (red and green of both tensors for the counts, the whole target once more for its min / max) over that time are set
  against the streaming figure of MI355X_MICROARCH.md (6.29 TB/s, float4 copy) -- reported, not gated.
* CodebookUsageTracker.update_counts at N = B * 16 * 16 vectors, L = 4 levels, K = 512 codes, alone and with the merge of the
  combinations that reading ``datasets`` triggers, against upstream's lines (flocoder/codebook_analysis.py:28-44) on the same indices.
* evaluate_model (is_midi, a tracker) on a U-Net and a VQVAE of the midi_vqgan.yaml shape against its parts timed separately; the same
  parts called by hand in one window, in evaluate_model's order, are timed as well (reported, not gated).

Expectations, each reported as met or MISSED: every kernel path is faster than the restatement of upstream's lines; evaluate_model costs
no more than the sum of its parts plus the spread (max - min over the windows) measured on those parts."""
import argparse
import json
import os
import sys
from collections import defaultdict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_ot import summary, windows  # noqa: E402

STREAM_TBS = 6.29        # MI355X_MICROARCH.md: HBM3E measured, float4 copy


def upstream_note_metrics(pred, target, threshold=0.4):
    """flocoder/metrics.py:362-455 for 3-channel rolls, restated: the same tensor operations, the Python loop over the batch, the fp32
    sums and the .item() calls."""
    minval, maxval = target.min(), target.max()
    pred_clamped = torch.clamp(pred.clone(), minval, maxval)
    target_unit = (target - minval) / (maxval - minval)
    pred_unit = (pred_clamped - minval) / (maxval - minval)
    pred_binary = torch.where(pred_unit > threshold, torch.ones_like(pred_unit), torch.zeros_like(pred_unit))
    target_binary = torch.where(target_unit > threshold, torch.ones_like(target_unit), torch.zeros_like(target_unit))
    metrics, metric_images = {}, {}
    for channel, name in enumerate(("onset", "sustain")):
        tot = [0, 0, 0, 0]
        imgs = [torch.zeros_like(pred_binary[:, 0]) for _ in range(4)]
        targpred = torch.zeros_like(target)
        for b in range(pred_binary.shape[0]):
            p, t = pred_binary[b, channel], target_binary[b, channel]
            planes = [(p == 1) & (t == 1), (p == 0) & (t == 0), (p == 1) & (t == 0), (p == 0) & (t == 1)]
            for k in range(4):
                tot[k] = tot[k] + torch.sum(planes[k]).float()
                imgs[k][b] = planes[k].float()
            targpred[b] = torch.cat([t.unsqueeze(0), p.unsqueeze(0), torch.zeros_like(t).unsqueeze(0)], dim=0)
        tp, tn, fp, fn = tot
        metrics.update({f"{name}_sensitivity": (tp / (tp + fn + 1e-8)).item(), f"{name}_specificity": (tn / (tn + fp + 1e-8)).item(),
                        f"{name}_precision": (tp / (tp + fp + 1e-8)).item(), f"{name}_f1": (2 * tp / (2 * tp + fp + fn + 1e-8)).item()})
        for k, key in enumerate(("tp", "tn", "fp", "fn")):
            metric_images[f"{name}_{key}"] = imgs[k].unsqueeze(1).repeat(1, 3, 1, 1)
        metric_images[f"{name}_targpred"] = targpred
    return metrics, metric_images


def upstream_update_counts(level_counts, combinations, indices):
    """flocoder/codebook_analysis.py:28-44, restated."""
    for level in range(len(level_counts)):
        level_indices = indices[:, level]
        counts = torch.bincount(level_indices, minlength=max(level_indices.max().item() + 1,
                                                             max(level_counts[level].keys()) + 1 if level_counts[level] else 1))
        for idx in torch.nonzero(counts > 0, as_tuple=True)[0]:
            level_counts[level][idx.item()] += counts[idx].item()
    unique_combos, combo_counts = torch.unique(indices, dim=0, return_counts=True)
    for combo, count in zip(unique_combos.cpu().numpy(), combo_counts.cpu().numpy()):
        combinations[tuple(combo)] += count


def device_time_ms(fn, reps, device):
    """ms per call of `fn` between two device events: the launches alone, no host wait inside."""
    fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(device)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize(device)
    return start.elapsed_time(stop) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--eval-batch", type=int, default=64)
    ap.add_argument("--eval-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py measures on an MI355X; no GPU found")
    from flocoder_amd import metrics as M
    from flocoder_amd import sampling as S
    from flocoder_amd.codebook_analysis import CodebookUsageTracker
    from flocoder_amd.codecs import VQVAE
    from flocoder_amd.unet import Unet
    device = torch.device("cuda", 0)
    expectations, note_rows, hist_rows = {}, [], []

    for B in args.batches:
        g = torch.Generator().manual_seed(B)
        target = torch.zeros(B, 3, 128, 128)
        roll = torch.rand(B, 128, 128, generator=g)
        target[:, 0], target[:, 1] = (roll > 0.97).float(), ((roll > 0.85) & (roll <= 0.97)).float()
        pred = (target + 0.35 * torch.randn(B, 3, 128, 128, generator=g)).to(device)
        target = target.to(device)
        ours, _ = M.calc_note_metrics(pred, target)
        theirs, _ = upstream_note_metrics(pred, target)
        assert all(abs(ours[k] - theirs[k]) <= 1e-6 for k in theirs), (ours, theirs)
        t = windows({"kernel": lambda r: M.calc_note_metrics(pred, target, images=False),
                     "kernel_with_images": lambda r: M.calc_note_metrics(pred, target),
                     "upstream_loop": lambda r: upstream_note_metrics(pred, target)}, args.windows, args.reps, device)
        dev_ms = device_time_ms(lambda: M.note_confusion(pred, target), 200, device)
        count_bytes, all_bytes = 4 * B * 128 * 128 * 4, 7 * B * 128 * 128 * 4
        row = {"batch": B, "shape": [B, 3, 128, 128], **{k: summary(v) for k, v in t.items()},
               "launches_alone": {"ms": round(dev_ms, 5), "bytes_read": all_bytes, "bytes_read_counting_pass": count_bytes,
                                  "achieved_TB_per_s": round(all_bytes / (1e-3 * dev_ms) / 1e12, 3), "streaming_TB_per_s": STREAM_TBS,
                                  "share_of_streaming": round(all_bytes / (1e-3 * dev_ms) / 1e12 / STREAM_TBS, 3),
                                  "what": "two memsets, the min / max launch and the counting launch, 200 calls between two device events"}}
        up = row["upstream_loop"]["median_ms"]
        expectations[f"calc_note_metrics B={B} faster than upstream's loop"] = row["kernel"]["median_ms"] < up
        expectations[f"calc_note_metrics with images B={B} faster than upstream's loop"] = row["kernel_with_images"]["median_ms"] < up
        note_rows.append(row)
        print(json.dumps(row), flush=True)

        n, levels, size = B * 16 * 16, 4, 512
        indices = torch.randint(0, size, (n, levels), generator=g)
        indices[: n // 2] = indices[: n // 2] % 7                       # half the vectors share few combinations, as trained latents do
        indices = indices.to(device)
        tracker = CodebookUsageTracker(levels, size)

        def update(r):
            if r == 0:
                tracker.reset_all()
            tracker.update_counts("val", indices)

        def update_and_merge(r):
            update(r)
            return tracker.datasets

        def upstream(r):
            upstream_update_counts([defaultdict(int) for _ in range(levels)], defaultdict(int), indices)
        update_and_merge(0), upstream(0)
        t = windows({"update_counts": update, "update_counts_and_merge": update_and_merge, "upstream_lines": upstream}, args.windows,
                    max(2, args.reps // 3), device)
        row = {"vectors": n, "levels": levels, "codebook_size": size, **{k: summary(v) for k, v in t.items()}}
        up = row["upstream_lines"]["median_ms"]
        expectations[f"update_counts N={n} faster than upstream's lines"] = row["update_counts"]["median_ms"] < up
        expectations[f"update_counts with the merge N={n} faster than upstream's lines"] = row["update_counts_and_merge"]["median_ms"] < up
        hist_rows.append(row)
        print(json.dumps(row), flush=True)

    # ---- evaluate_model against its parts
    B, levels, size = args.eval_batch, 4, 512
    torch.manual_seed(0)
    model = Unet(dim=32, dim_mults=(1, 2, 4, 8), channels=4, n_classes=0).to(device)
    codec = VQVAE(in_channels=3, hidden_channels=256, num_downsamples=3, internal_dim=128, vq_embedding_dim=4, vq_num_embeddings=size,
                  codebook_levels=levels).eval()
    g = torch.Generator().manual_seed(5)
    for i in range(levels):
        codec.vq.layers[i]._codebook.embed.copy_(torch.randn(1, size, 4, generator=g) * (0.5 ** i))
        codec.vq.layers[i]._codebook.initted.fill_(True)
    codec = codec.to(device)
    target = torch.randn(B, 4, 16, 16, generator=g).to(device)
    source = torch.randn(B, 4, 16, 16, generator=g).to(device)
    tracker = CodebookUsageTracker(levels, size)
    kw = dict(method="rk4", batch_size=B, n_steps=args.steps, n_classes=0, latent_shape=(4, 16, 16), is_midi=True, source=source)
    model.eval()
    pred_latents, decoded_pred, _ = S.sampler(model, codec, **kw)
    decoded_target = S.decode_latents(codec, target, True, False)

    def whole(r):
        if r == 0:
            tracker.reset_all()
        return S.evaluate_model(model, codec, 0, target, batch_size=B, n_steps=args.steps, is_midi=True, cb_tracker=tracker, source=source)

    def track(r):
        if r == 0:
            tracker.reset_all()
        for name, lat in (("val", target), ("gen", pred_latents)):
            tracker.update_counts(name, codec.vq.quantize_nchw(lat)[1])

    # (evaluate_model leaves the model in training mode, as upstream: the sampler part puts it back first, as evaluate_model does)
    parts = {"sampler": lambda r: (model.eval(), S.sampler(model, codec, **kw)), "decode_target": lambda r: S.decode_latents(codec, target, True, False),
             "compute_sample_metrics": lambda r: M.compute_sample_metrics(pred_latents, target, decoded_pred, decoded_target),
             "calc_note_metrics": lambda r: M.calc_note_metrics(decoded_pred, decoded_target, images=False),
             "quantize_and_track": track}

    def in_sequence(r):
        """The parts called by hand in evaluate_model's order inside ONE timed window: what the composition costs when every part finds
        the caches as its predecessor left them, which the parts timed on their own (each repeating itself) do not."""
        return [fn(r) for fn in parts.values()]
    whole(0)
    t = windows({"evaluate_model": whole, **parts, "parts_in_sequence": in_sequence}, args.windows, args.eval_reps, device)
    s = {k: summary(v) for k, v in t.items()}
    model.eval()
    parts_ms = sum(s[k]["median_ms"] for k in parts)
    allowed = parts_ms + sum(s[k]["spread_ms"] for k in parts)
    eval_row = {"batch": B, "rk4_steps": args.steps, "unet": "dim 32, mults (1, 2, 4, 8), 4 x 16 x 16 latents",
                "codec": "VQVAE 3 x 128 x 128, hidden 256, 3 downsamples, internal 128, 4 levels of 512 codes, random weights", **s,
                "sum_of_parts_ms": round(parts_ms, 4), "allowed_ms": round(allowed, 4)}
    expectations["evaluate_model <= its parts + the spread measured on the parts"] = s["evaluate_model"]["median_ms"] <= allowed
    print(json.dumps(eval_row), flush=True)

    doc = {"tool": "tools/bench_eval.py", "device": torch.cuda.get_device_name(device),
           "timing": f"{args.windows} alternating windows; host clock around device synchronisations; median, min, max, spread = max - min over "
                     f"windows; {args.reps} note-metric calls, {max(2, args.reps // 3)} counting calls, {args.eval_reps} evaluation calls per window; "
                     "every call ends in the host reading its numbers, except update_counts alone, which queues one launch",
           "expectations": {k: "met" if v else "MISSED" for k, v in expectations.items()},
           "note_metrics": note_rows, "codebook_counts": hist_rows, "evaluate_model": eval_row}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    missed = [k for k, v in expectations.items() if not v]
    print(f"wrote {args.out}; expectations missed: {missed if missed else 'none'}")


if __name__ == "__main__":
    main()
