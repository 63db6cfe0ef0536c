"""Parity metrics: host-side mirror of the sample metrics of ``flocoder/metrics.py``.

* ``g2rgb`` / ``rgb2g`` / ``to_uint8`` / ``normalize_recon`` -- the small tensor utilities (metrics.py:258-263,312-327,479-488);
* ``sinkhorn_loss`` (metrics.py:20-54) -- the debiased Sinkhorn divergence (p=2, blur 0.05, eps-scaling 0.5) on the device through
  ``fc_sinkhorn_divergence``: own HIP kernels restating geomloss's published algorithm (the package is absent: PARITY UNPINNED);
* ``fid_score`` (metrics.py:266-308) -- Frechet distance between Inception-pool features of real and generated images.  The
  statistics and the distance are computed here in float64; the feature network is a LOCAL TorchScript file (``inception=`` or
  ``$FLOCODER_FID_INCEPTION``) mapping uint8 images [B,3,H,W] to features [B,F] -- torchmetrics downloads its weights, this build
  never touches the network and raises FileNotFoundError without one;
* ``compute_sample_metrics`` (metrics.py:493-555) -- the same dictionary of numbers;
* ``calc_note_metrics`` (metrics.py:362-455, with ``targ_pred_mask_to_rgb`` / ``mask_to_rgb``, 330-340) -- onset / sustain sensitivity,
  specificity, precision and F1 of a piano roll against its target, and their images, from one streaming pass on the device
  (``fc_note_confusion``): exact int64 counts, ratios in fp64 on the host; ``region=`` restricts it to the pixels that were inpainted;
* ``prdc`` -- improved precision / recall and density / coverage of a generated set against a real one from exact k-NN radii on the
  device (``flocoder_amd.neighbors``; no upstream counterpart), optional in ``compute_sample_metrics`` (``prdc_k=``);
* ``frechet`` / ``frechet_px`` / ``kid`` / ``kid_px`` in ``compute_sample_metrics`` (``frechet=``, ``kid=``) and ``fid_score(solver="jacobi")``
  -- Frechet and kernel distances between the sample sets themselves on the device (``flocoder_amd.distances``; no upstream counterpart);
* ``bits_per_dim`` -- the flow's log-likelihood (``sampling.log_likelihood``) as bits per latent dimension (no upstream counterpart);
  ``bits_per_dim_stderr`` -- its standard error from a K-probe call's ``logp_stderr``.
"""
import ctypes as C
import os

import torch

from . import _binding as B


def rgb2g(img_t):
    """metrics.py:312-317 -- RGB piano roll -> grey float: black 0, red 1.0, green 0.5."""
    red = (img_t[-3] > 0.5).float()
    green = (img_t[-2] > 0.5).float() * 0.5
    return (red + green).unsqueeze(-3)


def g2rgb(gf_img, keep_gray=False):
    """metrics.py:319-327 -- grey float -> quantised RGB (0 black, 1 red, 0.5 green) or binary b/w."""
    if gf_img.shape[-3] == 3:
        return gf_img
    gf = gf_img.squeeze(-3)
    if keep_gray:
        return (gf > 0.5).float().unsqueeze(-3).repeat(1, 3, 1, 1)
    return torch.stack([(gf >= 0.75).float(), (torch.abs(gf - 0.5) < 0.25).float(), torch.zeros_like(gf)], dim=-3)


def targ_pred_mask_to_rgb(t_mask, p_mask):
    """metrics.py:330-334 -- target mask on red, prediction mask on green, blue zero: [H,W] x 2 -> [3,H,W]."""
    return torch.cat([t_mask.unsqueeze(0), p_mask.unsqueeze(0), torch.zeros_like(t_mask).unsqueeze(0)], dim=0)


def mask_to_rgb(mask, color=(1, 1, 1)):
    """metrics.py:336-340 -- [B,H,W] mask -> [B,3,H,W] in `color` (white by default)."""
    rgb = torch.zeros((mask.shape[0], 3, mask.shape[1], mask.shape[2]), device=mask.device)
    for i in range(3):
        rgb[:, i, :, :] = mask * color[i]
    return rgb


NOTE_NAMES = ('onset', 'sustain')


def note_ratios(tp, tn, fp, fn):
    """metrics.py:433-438 on exact totals, in fp64: Python ints give Python floats, int64 tensors give float64 tensors."""
    tp, tn, fp, fn = (v.double() if torch.is_tensor(v) else v for v in (tp, tn, fp, fn))
    return {'sensitivity': tp / (tp + fn + 1e-8), 'specificity': tn / (tn + fp + 1e-8), 'precision': tp / (tp + fp + 1e-8),
            'f1': 2 * tp / (2 * tp + fp + fn + 1e-8)}


def note_confusion(pred, target, threshold=0.4, minval=None, maxval=None, keep_gray=False, region=None, images=False):
    """The device half of ``calc_note_metrics`` (``fc_note_confusion``): counts int64 [2, B, 4] (onset | sustain; tp, tn, fp, fn per
    sample), still on the device and not waited for, plus with ``images`` the planes ``masks`` [2, 4, B, H, W] and ``overlay``
    [2, B, 3, H, W] (else None, None)."""
    if not (pred.is_cuda and target.is_cuda):
        raise RuntimeError("flocoder_amd.metrics.calc_note_metrics runs on MI355X (gfx950) only; there is no CPU path")
    if pred.dim() != 4 or target.dim() != 4 or pred.shape[0] != target.shape[0] or pred.shape[2:] != target.shape[2:]:
        raise ValueError(f"calc_note_metrics: pred {tuple(pred.shape)} and target {tuple(target.shape)} must be [B,C,H,W] of one B, H, W")
    if pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError("calc_note_metrics: pred and target must be float32")
    bsz, _, h, w = pred.shape
    pred = pred if pred.is_contiguous() else pred.contiguous()
    target = target if target.is_contiguous() else target.contiguous()
    if region is not None:
        if not region.is_cuda or tuple(region.shape) != (bsz, 1, h, w):
            raise ValueError(f"calc_note_metrics: region must be a device tensor [B,1,H,W] = {(bsz, 1, h, w)}")
        region = region.float().contiguous()
    dev = pred.device
    counts = torch.empty(2, bsz, 4, dtype=torch.int64, device=dev)
    ws = torch.empty(4, dtype=torch.int32, device=dev)
    masks = torch.empty(2, 4, bsz, h, w, dtype=torch.float32, device=dev) if images else None
    overlay = torch.empty(2, bsz, 3, h, w, dtype=torch.float32, device=dev) if images else None
    with torch.cuda.device(dev):
        B.check(B.lib().fc_note_confusion(B.ptr(pred), pred.shape[1], B.ptr(target), target.shape[1], B.ptr(region), bsz, h, w,
                                          float(threshold), 0.0 if minval is None else float(minval), int(minval is None),
                                          0.0 if maxval is None else float(maxval), int(maxval is None), int(bool(keep_gray)),
                                          B.ptr(ws), B.ptr(counts), B.ptr(masks), B.ptr(overlay), B.current_stream(dev)))
    return counts, masks, overlay


def calc_note_metrics(pred, target, threshold=0.4, minval=None, maxval=None, keep_gray=False, debug=False, *, region=None,
                      per_sample=False, images=True):
    """metrics.py:362-455 -- onset / sustain sensitivity, specificity, precision and F1 of a piano roll against its target, and the
    images that go with them, from one streaming pass on the device (``fc_note_confusion``: upstream's g2rgb, min / max of the whole
    converted target, clamp, rescale and ``> threshold`` in fp32 and in its order of operations) instead of a Python loop over the batch.
    Returns ``(metrics, metric_images)`` with upstream's keys: ``{onset,sustain}_{sensitivity,specificity,precision,f1}`` as Python
    floats and ``{onset,sustain}_{tp,tn,fp,fn,targpred}`` as [B,3,H,W] tensors (the four masks are broadcast views of the [B,H,W] planes
    the kernel wrote, where upstream repeats them).

    Differences, all deliberate: the counts are exact int64 totals and the ratios are formed from them on the host in fp64, where
    upstream sums in fp32 (not exact above 2^24 pixels) and divides in fp32 -- the two agree to fp32 rounding; ``minval`` / ``maxval``
    given as tensors are read as numbers; the rescaling is an IEEE division by the range, as torch does it on the CPU and, with a
    derived range, on the GPU (given two Python numbers, torch's GPU kernel multiplies by the reciprocal instead, one rounding away).  Keyword-only extensions: ``region`` [B,1,H,W] restricts every count (and image) to the
    pixels where region > 0.5, e.g. the part of a roll that was inpainted; ``per_sample=True`` adds ``metrics['per_sample']`` (the
    eight ratios as [B] float64 device tensors) and ``metrics['counts']`` (int64 [2,B,4]: onset | sustain; tp, tn, fp, fn);
    ``images=False`` skips the image writes and returns ``{}``.  One device-to-host copy (the 2 x 4 totals) ends the call."""
    if debug:
        print(f"calc_note_metrics: pred.shape = {tuple(pred.shape)}, target.shape = {tuple(target.shape)}")
    counts, masks, overlay = note_confusion(pred, target, threshold, minval, maxval, keep_gray, region, images)
    totals = counts.sum(dim=1).tolist()
    metrics, metric_images = {}, {}
    for i, name in enumerate(NOTE_NAMES):
        tp, tn, fp, fn = totals[i]
        if debug:
            print(f" {name}: tp, tn, fp, fn =", [tp, tn, fp, fn])
        metrics.update({f'{name}_{k}': v for k, v in note_ratios(tp, tn, fp, fn).items()})
        if images:
            bsz, h, w = masks.shape[2:]
            metric_images.update({f'{name}_{k}': masks[i, q].unsqueeze(1).expand(bsz, 3, h, w) for q, k in enumerate(('tp', 'tn', 'fp', 'fn'))})
            metric_images[f'{name}_targpred'] = overlay[i]
    if per_sample:
        metrics['counts'] = counts
        metrics['per_sample'] = {f'{name}_{k}': v for i, name in enumerate(NOTE_NAMES)
                                 for k, v in note_ratios(*counts[i].unbind(dim=1)).items()}
    return metrics, metric_images


def to_uint8(x):
    """metrics.py:258-263 -- per-image min/max stretch to uint8."""
    x = x.clone().detach()
    x -= x.amin(dim=(1, 2, 3), keepdim=True)
    x /= x.amax(dim=(1, 2, 3), keepdim=True).clamp(min=1e-5)
    return (x * 255).clamp(0, 255).to(torch.uint8)


def normalize_recon(orig, recon):
    """metrics.py:479-488 -- rescale each RGB channel of `recon` to the range of `orig` (vectorised; in place like upstream)."""
    o_min, o_max = orig[:, :3].amin(dim=(2, 3), keepdim=True), orig[:, :3].amax(dim=(2, 3), keepdim=True)
    r_min, r_max = recon[:, :3].amin(dim=(2, 3), keepdim=True), recon[:, :3].amax(dim=(2, 3), keepdim=True)
    ok = r_max > r_min
    scaled = (recon[:, :3] - r_min) / (r_max - r_min).clamp_min(1e-30) * (o_max - o_min) + o_min
    recon[:, :3] = torch.where(ok, scaled, recon[:, :3])
    return recon


def rel_l2(a, b):
    """||a-b|| / ||b|| in fp64 -- the parity gate of BASELINE.md section 4."""
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def bits_per_dim(logp, numel):
    """Bits per dimension of ``sampling.log_likelihood``'s ``logp`` (natural log, per sample) over ``numel`` = C*H*W unknowns:
    ``-logp / (numel ln 2)``.  For latents of a codec (SD-VAE, VQVAE) these are bits per LATENT dimension: the codec's own change of
    volume is not in it, so the figure compares flows over the same latent space, not models of the pixels."""
    import math
    return -logp / (float(numel) * math.log(2.0))


def bits_per_dim_stderr(stderr, numel):
    """``sampling.log_likelihood(..., return_info=True)``'s ``logp_stderr`` (nats) as bits per dimension: ``stderr / (numel ln 2)``, the
    standard error of ``bits_per_dim`` of the same sample from the divergence estimator's variance."""
    import math
    return stderr / (float(numel) * math.log(2.0))


def sample_stats(pred_latents, target_latents, decoded_pred, decoded_target):
    """The third-party-free part of compute_sample_metrics (metrics.py:530-545)."""
    n = min(pred_latents.shape[0], target_latents.shape[0])
    f = torch.nn.functional.mse_loss
    return {
        'mse': f(pred_latents[:n], target_latents[:n]).item(), 'mse_px': f(decoded_pred, decoded_target).item(),
        'pred_mean': pred_latents.mean().item(), 'targ_mean': target_latents.mean().item(),
        'pred_std': pred_latents.std().item(), 'targ_std': target_latents.std().item(),
        'pred_px_mean': decoded_pred.mean().item(), 'targ_px_mean': decoded_target.mean().item(),
        'pred_px_std': decoded_pred.std().item(), 'targ_px_std': decoded_target.std().item(),
    }


# ------------------------------------------------------------------------------------------------ sinkhorn (metrics.py:20-54)
def sinkhorn_divergence(x, y, blur: float = 0.05, scaling: float = 0.5, diameter=None, return_info: bool = False):
    """S_eps between point clouds x [N,...] and y [M,...] (flattened per sample), uniform weights, cost |x-y|^2/2, on the GPU."""
    if not (x.is_cuda and y.is_cuda):
        raise RuntimeError("flocoder_amd.metrics.sinkhorn_divergence runs on MI355X (gfx950) only; there is no CPU path "
                           "(the CPU restatement under oracle/ is test infrastructure)")
    xf = x.reshape(x.shape[0], -1).float().contiguous()
    yf = y.reshape(y.shape[0], -1).float().contiguous()
    if xf.shape[1] != yf.shape[1]:
        raise ValueError("sinkhorn: both clouds must live in the same space")
    val, diam, its = C.c_double(0), C.c_double(0), C.c_int(0)
    B.check(B.lib().fc_sinkhorn_divergence(B.ptr(xf), B.ptr(yf), xf.shape[0], yf.shape[0], xf.shape[1], float(blur), float(scaling),
                                           float(diameter) if diameter else 0.0, C.byref(val), C.byref(diam), C.byref(its),
                                           B.current_stream(xf.device)))
    return (val.value, {"diameter": diam.value, "iterations": its.value}) if return_info else val.value


def sinkhorn_loss_chunked(target, gen, chunk_size=256, device='cuda'):
    """metrics.py:20-38: the mean of per-chunk divergences."""
    assert target.shape == gen.shape, f"target.shape {target.shape} != gen.shape {gen.shape}"
    vals = []
    for i in range(0, target.shape[0], chunk_size):
        vals.append(sinkhorn_divergence(target[i:i + chunk_size].to(device), gen[i:i + chunk_size].to(device)))
    return sum(vals) / len(vals)


def sinkhorn_loss(target, gen, max_B=None, device='cuda', chunk=False, debug=False):
    """metrics.py:40-54: SamplesLoss("sinkhorn", p=2, blur=0.05)(target, gen) on samples flattened to vectors; a Python float."""
    if chunk:
        return sinkhorn_loss_chunked(target, gen, device=device)
    assert target.shape == gen.shape, f"target.shape {target.shape} != gen.shape {gen.shape}"
    n = target.shape[0] if max_B is None else min(target.shape[0], max_B)
    return sinkhorn_divergence(target[:n].to(device), gen[:n].to(device))


# ------------------------------------------------------------------------------------------------ FID (metrics.py:266-308)
_INCEPTION = {}


def load_feature_extractor(path=None, device='cuda'):
    """The Inception-v3 pool3 network torchmetrics fetches, from a LOCAL TorchScript file (uint8 [B,3,H,W] -> float [B,F])."""
    path = path or os.environ.get("FLOCODER_FID_INCEPTION")
    if not path:
        raise FileNotFoundError("fid_score: no local Inception feature extractor.  Pass inception=<TorchScript file | callable> or set "
                                "FLOCODER_FID_INCEPTION (torchmetrics downloads its weights; this build never touches the network).")
    if not os.path.exists(path):
        raise FileNotFoundError(f"fid_score: feature extractor {path} does not exist")
    key = (os.path.abspath(path), str(device))
    if key not in _INCEPTION:
        _INCEPTION[key] = torch.jit.load(path, map_location=device).eval()
    return _INCEPTION[key]


class FrechetStatistics:
    """Running sum and sum of outer products of feature vectors in float64 (what torchmetrics' FrechetInceptionDistance keeps)."""

    def __init__(self):
        self.n, self.s, self.ss = 0, None, None

    def update(self, feats: torch.Tensor):
        f = feats.reshape(feats.shape[0], -1).double()
        if self.s is None:
            self.s = torch.zeros(f.shape[1], dtype=torch.float64, device=f.device)
            self.ss = torch.zeros(f.shape[1], f.shape[1], dtype=torch.float64, device=f.device)
        self.n += f.shape[0]
        self.s += f.sum(0)
        self.ss += f.t() @ f

    def moments(self):
        if self.n < 2:
            raise RuntimeError("FID needs at least two samples per side")
        mu = self.s / self.n
        return mu, (self.ss - self.n * torch.outer(mu, mu)) / (self.n - 1)


def frechet_distance(mu1, sigma1, mu2, sigma2) -> float:
    """|mu1 - mu2|^2 + tr(S1) + tr(S2) - 2 tr(sqrt(S1 S2)), the matrix square root through the eigenvalues of S1 S2."""
    a = (mu1 - mu2).square().sum()
    b = sigma1.trace() + sigma2.trace()
    c = torch.linalg.eigvals((sigma1 @ sigma2).cpu()).sqrt().real.sum().to(a.device)
    return float(a + b - 2 * c)


@torch.no_grad()
def fid_score(real, fake, device='cuda', chunk=False, inception=None, chunk_size=256, solver="eig"):
    """metrics.py:266-308.  ``inception``: a callable uint8 [B,3,H,W] -> features, or a TorchScript path (see load_feature_extractor).
    ``solver="jacobi"`` keeps the extractor's features on the device and returns ``distances.frechet_distance_sets`` of them (no F x F
    covariance, no host eigenvalues; sample counts within that function's limits); ``"eig"`` is the moment form above.
    ``solver="moments"`` feeds every chunk's features straight into two ``distances.FrechetMoments`` and returns
    ``distances.frechet_distance_moments`` of them: the features are never held, any number of samples, at most 4096 features."""
    if solver not in ("eig", "jacobi", "moments"):
        raise ValueError(f"fid_score: solver must be 'eig', 'jacobi' or 'moments', got {solver!r}")
    net = inception if callable(inception) else load_feature_extractor(inception, device)
    if solver == "moments":
        from . import distances as D
        states = (D.FrechetMoments(), D.FrechetMoments())
        step = chunk_size if chunk else max(real.shape[0], fake.shape[0])
        for side, imgs in enumerate((real, fake)):
            for i in range(0, imgs.shape[0], step):
                u8 = to_uint8(imgs[i:i + step].to(device))
                if u8.shape[1] == 1:
                    u8 = u8.repeat(1, 3, 1, 1)
                states[side].update(net(u8))
        return D.frechet_distance_moments(states[0], states[1])
    if solver == "jacobi":
        from . import distances as D
        step = chunk_size if chunk else max(real.shape[0], fake.shape[0])
        feats = []
        for imgs in (real, fake):
            parts = []
            for i in range(0, imgs.shape[0], step):
                u8 = to_uint8(imgs[i:i + step].to(device))
                if u8.shape[1] == 1:
                    u8 = u8.repeat(1, 3, 1, 1)
                parts.append(net(u8).reshape(u8.shape[0], -1).float())
            feats.append(torch.cat(parts))
        return D.frechet_distance_sets(feats[0], feats[1])
    stats = (FrechetStatistics(), FrechetStatistics())
    step = chunk_size if chunk else max(real.shape[0], fake.shape[0])
    for side, imgs in enumerate((real, fake)):
        for i in range(0, imgs.shape[0], step):
            u8 = to_uint8(imgs[i:i + step].to(device))
            if u8.shape[1] == 1:
                u8 = u8.repeat(1, 3, 1, 1)
            stats[side].update(net(u8))
    return frechet_distance(*stats[0].moments(), *stats[1].moments())


# ------------------------------------------------------------------------------------------------ precision / recall / density / coverage
@torch.no_grad()
def prdc(real, fake, k=5):
    """Improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) between the sample sets
    ``real`` [N,...] and ``fake`` [M,...] (flattened per sample), on squared distances -- every comparison is monotone, so squared and
    plain distances agree.  With r_real[i] the d2 of real i's k-th neighbour among the OTHER real rows, r_fake[j] likewise:

        precision = mean_j [exists i: d2(fake_j, real_i) <= r_real[i]]      recall   = mean_i [exists j: d2(real_i, fake_j) <= r_fake[j]]
        density   = sum_j #{i: d2(fake_j, real_i) <= r_real[i]} / (k M)     coverage = mean_i [min_j d2(real_i, fake_j) <= r_real[i]]

    Five calls into ``flocoder_amd.neighbors`` (two self-``knn``, two ``ball_counts``, one cross ``knn`` with k = 1), exact and
    deterministic; a set with fewer than k + 1 rows has radius +inf.  Nothing is read on the host until the four numbers are.  Returns
    a dict of Python floats."""
    from . import neighbors as NB
    if not (real.is_cuda and fake.is_cuda):
        raise RuntimeError("flocoder_amd.metrics.prdc runs on MI355X (gfx950) only; there is no CPU path")
    n, m = real.shape[0], fake.shape[0]
    if n < 1 or m < 1:
        raise ValueError(f"prdc: both sets need at least one sample, got {n} and {m}")
    dev = real.device
    r_real = NB.knn(real, real, k, query_ids=torch.arange(n, device=dev))[0][:, k - 1].contiguous()
    r_fake = NB.knn(fake, fake, k, query_ids=torch.arange(m, device=dev))[0][:, k - 1].contiguous()
    in_real = NB.ball_counts(fake, real, r_real)                     # per fake sample: the real balls it lies in
    in_fake = NB.ball_counts(real, fake, r_fake)
    nearest_fake = NB.knn(real, fake, 1)[0][:, 0]
    # exact integer counts, one fp64 division each: the numbers are count / size to the last bit
    counts = torch.stack([(in_real > 0).sum(), (in_fake > 0).sum(), in_real.sum(dtype=torch.int64), (nearest_fake <= r_real).sum()]).double()
    out = (counts / torch.tensor([m, n, k * m, n], dtype=torch.float64, device=dev)).tolist()
    return dict(zip(('precision', 'recall', 'density', 'coverage'), out))


@torch.no_grad()
def compute_sample_metrics(pred_latents, target_latents, decoded_pred, decoded_target, debug=False, inception=None, *, prdc_k=None,
                           frechet=False, kid=False):
    """metrics.py:493-555: the dictionary evaluate_model logs.  'FID_px' is present only when a local feature extractor is (it is
    the one entry that needs third-party weights); everything else is computed unconditionally.  Keyword-only ``prdc_k`` (an integer)
    adds ``prdc/{precision,recall,density,coverage}`` of ``prdc(target_latents, pred_latents, prdc_k)``: the target latents are the real set.
    Keyword-only ``frechet`` / ``kid`` add ``frechet`` and ``frechet_px`` / ``kid`` and ``kid_px``: ``distances.frechet_distance_sets`` /
    ``distances.kernel_distance`` of the target latents against the generated ones and of the decoded images, on the sets that
    ``sinkhorn`` / ``sinkhorn_px`` compare -- raw latents and pixels, no feature network."""
    n = min(pred_latents.shape[0], target_latents.shape[0])
    decoded_pred = normalize_recon(decoded_target, decoded_pred)
    out = {}
    if inception is not None or os.environ.get("FLOCODER_FID_INCEPTION"):
        out['FID_px'] = fid_score(decoded_target, decoded_pred, device=decoded_pred.device, inception=inception)
    out['sinkhorn'] = sinkhorn_loss(target_latents[:n], pred_latents[:n], device=pred_latents.device)
    out['sinkhorn_px'] = sinkhorn_loss(decoded_target, decoded_pred, device=decoded_pred.device)
    out.update(sample_stats(pred_latents, target_latents, decoded_pred, decoded_target))
    if prdc_k is not None:
        out.update({f'prdc/{key}': v for key, v in prdc(target_latents, pred_latents, prdc_k).items()})
    if frechet or kid:
        from . import distances as D
        for on, name, fn in ((frechet, 'frechet', D.frechet_distance_sets), (kid, 'kid', D.kernel_distance)):
            if on:
                out[name] = fn(target_latents[:n], pred_latents[:n])
                out[f'{name}_px'] = fn(decoded_target, decoded_pred)
    return out
