"""Mini-batch OT pairing: host-side mirror of ``flocoder/ot.py`` (ot.py:63-84).  Upstream's wrapper hard-wires the greedy matcher
(ot.py:80-84) and carries its POT / torchcfm variants as dead code; here the greedy matcher (``fc_ot_pairing``) stays the default
and the exact mini-batch coupling of the OT-CFM literature -- the permutation minimising the summed squared distance, what torchcfm's
``OTPlanSampler("exact")`` solves -- is ``method="exact"`` (``fc_ot_pairing_exact``: squared-distance matrix and a shortest-augmenting-
path assignment solver, both on the caller's stream, no host round trip).  Entropic (Sinkhorn) plans and sampling pairs with
replacement from a plan are not built."""
import torch

from . import _binding as B
from ._ops import ot_pairing_exact


def compute_ot_pairing_approximate(source, target):
    """ot.py:63-78 on the GPU: L2 distance matrix, then the sequential greedy sweep (first minimum among unused targets).
    Returns an int64 permutation on the inputs' device."""
    if not source.is_cuda:
        raise RuntimeError("flocoder_amd.compute_ot_pairing runs on MI355X (gfx950) only; there is no CPU path")
    bsz = source.shape[0]
    s = source.reshape(bsz, -1).contiguous().float()
    t = target.reshape(bsz, -1).contiguous().float()
    dist = torch.empty(bsz, bsz, device=s.device, dtype=torch.float32)
    perm = torch.empty(bsz, device=s.device, dtype=torch.int64)
    B.check(B.lib().fc_ot_pairing(B.ptr(s), B.ptr(t), bsz, s.shape[1], B.ptr(dist), B.ptr(perm), B.current_stream(s.device)))
    return perm


def compute_ot_pairing_exact(source, target, return_info=False):
    """The permutation minimising sum_i |source_i - target_perm[i]|^2 (batch in [1, 1024]), int64 on the inputs' device.  With
    ``return_info`` also {"cost": the fp32 squared-distance matrix [B,B] (non-finite entries stored as FLT_MAX), "u", "v": the
    optimal fp64 duals, u_i + v_j <= cost_ij with equality on the pairing; a pair that holds a FLT_MAX entry, or was reached over one,
    is exempt: csrc/ot.hip, "Sentinels and the duals"}."""
    if not source.is_cuda:
        raise RuntimeError("flocoder_amd.compute_ot_pairing_exact runs on MI355X (gfx950) only; there is no CPU path")
    bsz = source.shape[0]
    if not 1 <= bsz <= 1024:                          # the library's FC_E_SHAPE, before an empty batch reaches reshape
        raise ValueError(f"flocoder_amd: compute_ot_pairing_exact: batch must be in [1, 1024], got {bsz}")
    perm, cost, duals = ot_pairing_exact(source, target, want_duals=return_info)
    if return_info:
        return perm, {"cost": cost, "u": duals[0], "v": duals[1]}
    return perm


def compute_ot_pairing(source, target, debug=False, method="greedy"):
    """ot.py:80-84.  ``method``: "greedy" (upstream's matcher, the default) or "exact"."""
    if method == "greedy":
        return compute_ot_pairing_approximate(source, target)
    if method == "exact":
        return compute_ot_pairing_exact(source, target)
    raise ValueError(f"compute_ot_pairing: method must be 'greedy' or 'exact', got {method!r}")


def pairing_cost(source, target, perm=None):
    """mean_i |source_i - target_perm[i]|^2 as a 0-d device tensor (``perm=None``: the identity): the figure that shows in a training
    log whether the pairing shortens the couplings."""
    bsz = source.shape[0]
    s = source.reshape(bsz, -1).float()
    t = target.reshape(bsz, -1).float()
    if perm is not None:
        t = t[perm.to(t.device)]
    return (s - t).square().sum(1).mean()
