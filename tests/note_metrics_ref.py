"""Yardstick for ``flocoder_amd.metrics.calc_note_metrics``: upstream's ``calc_note_metrics`` (flocoder/metrics.py:362-455, with its
``g2rgb``, 319-327) restated in plain torch, runnable on the CPU.  The tensor arithmetic is upstream's, operation for operation, in
fp32; what is counted is kept as int64 per sample, and the ratios are given twice: in fp64 from the integer totals (what the package
promises) and in fp32 the way upstream forms them (float sums of the per-sample counts, fp32 division).  ``region`` is the package's
extension: a pixel counts where region > 0.5 and is zero in every image elsewhere.  The implementation does not import this file."""
import torch

NAMES = ("onset", "sustain")


def g2rgb(gf_img, keep_gray=False):
    if gf_img.shape[-3] == 3:
        return gf_img
    gf = gf_img.squeeze(-3)
    if keep_gray:
        return (gf > 0.5).float().unsqueeze(-3).repeat(1, 3, 1, 1)
    return torch.stack([(gf >= 0.75).float(), (torch.abs(gf - 0.5) < 0.25).float(), torch.zeros_like(gf)], dim=-3)


def binarise(pred, target, threshold=0.4, minval=None, maxval=None, keep_gray=False):
    """metrics.py:364-374: (pred_binary, target_binary), both [B,3,H,W] of 0 / 1."""
    pred, target = g2rgb(pred, keep_gray=keep_gray), g2rgb(target, keep_gray=keep_gray)
    if minval is None:
        minval = target.min()
    if maxval is None:
        maxval = target.max()
    pred_clamped = torch.clamp(pred.clone(), minval, maxval)
    target_unit = (target - minval) / (maxval - minval)
    pred_unit = (pred_clamped - minval) / (maxval - minval)
    pred_binary = torch.where(pred_unit > threshold, torch.ones_like(pred_unit), torch.zeros_like(pred_unit))
    target_binary = torch.where(target_unit > threshold, torch.ones_like(target_unit), torch.zeros_like(target_unit))
    return pred_binary, target_binary


def ratios64(tp, tn, fp, fn):
    """The four ratios in Python floats (fp64) from integer totals, upstream's 1e-8 in the denominators."""
    return {"sensitivity": tp / (tp + fn + 1e-8), "specificity": tn / (tn + fp + 1e-8), "precision": tp / (tp + fp + 1e-8),
            "f1": 2 * tp / (2 * tp + fp + fn + 1e-8)}


def ratios32(per_sample_counts):
    """metrics.py:415-418,434-437: fp32 sums of the per-sample counts, fp32 ratios.  per_sample_counts: int64 [B,4] tp, tn, fp, fn."""
    tot = [0, 0, 0, 0]
    for row in per_sample_counts:
        for k in range(4):
            tot[k] = tot[k] + row[k].float()
    tp, tn, fp, fn = tot
    return {"sensitivity": (tp / (tp + fn + 1e-8)).item(), "specificity": (tn / (tn + fp + 1e-8)).item(),
            "precision": (tp / (tp + fp + 1e-8)).item(), "f1": (2 * tp / (2 * tp + fp + fn + 1e-8)).item()}


def note_metrics_ref(pred, target, threshold=0.4, minval=None, maxval=None, keep_gray=False, region=None):
    """-> dict: ``counts`` int64 [2,B,4] (onset | sustain; tp, tn, fp, fn per sample), ``metrics`` (fp64 ratios, upstream's keys),
    ``metrics32`` (upstream's fp32 form), ``images`` (upstream's keys: four [B,3,H,W] masks and the target / pred overlay per name)."""
    pred_binary, target_binary = binarise(pred, target, threshold, minval, maxval, keep_gray)
    bsz = pred_binary.shape[0]
    inside = torch.ones_like(pred_binary[:, 0], dtype=torch.bool) if region is None else region[:, 0] > 0.5
    counts = torch.zeros(2, bsz, 4, dtype=torch.int64)
    metrics, metrics32, images = {}, {}, {}
    for i, name in enumerate(NAMES):
        p, t = pred_binary[:, i] == 1, target_binary[:, i] == 1
        planes = [p & t & inside, ~p & ~t & inside, p & ~t & inside, ~p & t & inside]
        for k, plane in enumerate(planes):
            counts[i, :, k] = plane.flatten(1).sum(dim=1)
        tp, tn, fp, fn = (int(v) for v in counts[i].sum(dim=0))
        metrics.update({f"{name}_{k}": v for k, v in ratios64(tp, tn, fp, fn).items()})
        metrics32.update({f"{name}_{k}": v for k, v in ratios32(counts[i]).items()})
        for k, plane in zip(("tp", "tn", "fp", "fn"), planes):
            images[f"{name}_{k}"] = plane.float().unsqueeze(1).repeat(1, 3, 1, 1)
        images[f"{name}_targpred"] = torch.stack([(t & inside).float(), (p & inside).float(), torch.zeros_like(pred_binary[:, 0])], dim=1)
    return {"counts": counts, "metrics": metrics, "metrics32": metrics32, "images": images}
