"""Mini-batch OT couplings: host-side mirror of ``flocoder/ot.py`` (ot.py:63-84).  Upstream's wrapper hard-wires the greedy matcher
(ot.py:80-84) and carries its POT / torchcfm variants as dead code; here all of them run on the device, on the caller's stream and
without a host round trip:

- ``method="greedy"`` (``fc_ot_pairing``), upstream's matcher and the default;
- ``method="exact"`` (``fc_ot_pairing_exact``): the permutation minimising the summed squared distance, what torchcfm's
  ``OTPlanSampler("exact")`` solves -- squared-distance matrix and a shortest-augmenting-path assignment solver;
- ``method="sinkhorn"``: upstream's ``compute_ot_pairing_vanilla`` -- an entropic plan (``compute_ot_plan``, ``fc_ot_plan_sinkhorn``)
  turned into a permutation by the row-by-row "largest entry among the unused targets" sweep (``fc_ot_plan_pairing``);
- ``compute_ot_plan`` / ``sample_plan`` / ``OTPlanSampler``: the plan itself and index pairs drawn from it with replacement
  (``fc_ot_sample_plan``), upstream's ``compute_ot_pairing_torchcfm`` and what the OT-CFM literature trains with.

The entropic solver is POT's ``sinkhorn_knopp`` restated in the log domain (csrc/ot_plan.hip): kernel-form Sinkhorn forms
``exp(-M / reg)``, which for squared distances around 8000 (4 x 32 x 32 latents) and upstream's ``reg`` of 0.05 - 0.1 is an all-zero
matrix -- torchcfm then falls back to the uniform plan, i.e. to no pairing at all.  The log-domain iteration has no such limit, but its
iteration count grows with max(cost) / reg: on raw squared distances it does not converge within the default 1000 iterations;
``normalize_cost=True`` (torchcfm's option) is what makes ``reg`` comparable across data sets.  Neither POT nor torchcfm is a
dependency: the plan is checked by its own certificate (Gibbs form, marginals: tests/test_gpu_ot_sinkhorn.py).

Not built: rectangular batches, non-uniform marginals, unbalanced / partial OT, eps-scaling, and pairing across data-parallel ranks."""
import torch

from . import _binding as B
from ._ops import ot_pairing_exact, ot_plan_pairing, ot_plan_sinkhorn, ot_sample_plan


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


def compute_ot_plan(source, target, reg=0.05, normalize_cost=False, max_iter=1000, stop_thr=1e-9, return_info=False):
    """The entropic transport plan between the two batches (uniform marginals, squared Euclidean cost, batch in [1, 1024]): fp32
    ``[B,B]`` on the inputs' device, entries summing to 1, row sums 1/B.  ``normalize_cost`` divides the cost matrix by its maximum
    first.  With ``return_info`` also {"cost": the matrix the solver saw, "f", "g": the fp64 potentials, plan_ij = exp((f_i + g_j -
    cost_ij) / reg), "iterations", "converged", "err": 0-d device tensors -- the iterations run (int64), whether the column marginal's
    L2 error fell below ``stop_thr`` within ``max_iter`` (bool), and that error at the last check}.  Nothing here reads the device back."""
    bsz = source.shape[0]
    if not 1 <= bsz <= 1024:
        raise ValueError(f"flocoder_amd: compute_ot_plan: batch must be in [1, 1024], got {bsz}")
    if target.shape[0] != bsz:
        raise ValueError(f"flocoder_amd: compute_ot_plan: source and target batches differ ({bsz} and {target.shape[0]})")
    if not reg > 0 or not stop_thr >= 0 or not 1 <= int(max_iter) <= 10000:
        raise ValueError(f"flocoder_amd: compute_ot_plan: need reg > 0, stop_thr >= 0 and max_iter in [1, 10000], got {reg}, {stop_thr}, {max_iter}")
    if not source.is_cuda:
        raise RuntimeError("flocoder_amd.compute_ot_plan runs on MI355X (gfx950) only; there is no CPU path")
    plan, cost, duals, info = ot_plan_sinkhorn(source, target, reg, normalize_cost, max_iter, stop_thr)
    if return_info:
        return plan, {"cost": cost, "f": duals[0], "g": duals[1], "iterations": info[0].to(torch.int64), "converged": info[1] != 0,
                      "err": info[2]}
    return plan


def sample_plan(plan, n_pairs=None, seed=0, draw_index=0):
    """``n_pairs`` (default: the batch; at most 65536) index pairs ``(i, j)``, int64 on the plan's device, drawn with replacement from the
    plan read as a categorical over its cells: torchcfm's ``OTPlanSampler.sample_map``.  The pairs are a function of (plan, seed,
    draw_index, position k) alone -- ``flocoder_amd.noise.plan_uniforms`` gives the uniforms on the host."""
    if plan.dim() != 2 or plan.shape[0] != plan.shape[1] or not 1 <= plan.shape[0] <= 1024:
        raise ValueError(f"flocoder_amd: sample_plan: plan must be [B,B] with B in [1, 1024], got {tuple(plan.shape)}")
    n_pairs = plan.shape[0] if n_pairs is None else int(n_pairs)
    if not 1 <= n_pairs <= 65536:
        raise ValueError(f"flocoder_amd: sample_plan: n_pairs must be in [1, 65536], got {n_pairs}")
    if not 0 <= int(draw_index) <= 0xffffffff:
        raise ValueError("flocoder_amd: sample_plan: draw_index is a 32-bit counter word")
    if not plan.is_cuda:
        raise RuntimeError("flocoder_amd.sample_plan runs on MI355X (gfx950) only; there is no CPU path")
    return ot_sample_plan(plan, n_pairs, seed, draw_index)


class OTPlanSampler:
    """torchcfm's ``OTPlanSampler`` surface on the device.  ``method``: "exact" -- the permutation plan, 1/B on the exact pairing -- or
    "sinkhorn" -- the entropic plan with ``reg`` (and ``normalize_cost``).  Draws are counter-based: the object counts them
    (``draw_index``, one per ``sample_map`` / ``sample_plan`` / ``sample_plan_with_labels`` call), so a run resumed with the same
    ``seed`` and the saved ``draw_index`` draws what the uninterrupted run would have."""

    def __init__(self, method="exact", reg=0.05, normalize_cost=False, seed=0, draw_index=0):
        if method not in ("exact", "sinkhorn"):
            raise ValueError(f"OTPlanSampler: method must be 'exact' or 'sinkhorn', got {method!r}")
        if not reg > 0:
            raise ValueError(f"OTPlanSampler: reg must be positive, got {reg}")
        if not 0 <= int(draw_index) <= 0xffffffff:
            raise ValueError("OTPlanSampler: draw_index is a 32-bit counter word")
        self.method, self.reg, self.normalize_cost, self.seed = method, float(reg), bool(normalize_cost), int(seed)
        self.draw_index = int(draw_index)

    def state_dict(self):
        return {"seed": self.seed, "draw_index": self.draw_index}

    def load_state_dict(self, state):
        self.seed, self.draw_index = int(state["seed"]), int(state["draw_index"])

    def get_map(self, x0, x1):
        """The plan between the two batches, fp32 [B,B] on their device."""
        if x0.shape[0] != x1.shape[0]:
            raise ValueError(f"OTPlanSampler: the batches differ ({x0.shape[0]} and {x1.shape[0]}); rectangular plans are not built")
        if self.method == "sinkhorn":
            return compute_ot_plan(x0, x1, reg=self.reg, normalize_cost=self.normalize_cost)
        perm = compute_ot_pairing_exact(x0, x1)
        bsz = perm.shape[0]
        plan = torch.zeros(bsz, bsz, device=perm.device, dtype=torch.float32)
        plan[torch.arange(bsz, device=perm.device), perm] = 1.0 / bsz
        return plan

    def _next_draw(self):
        if self.draw_index > 0xffffffff:
            raise ValueError("OTPlanSampler: the 32-bit draw counter is exhausted; continue with another seed")
        d = self.draw_index
        self.draw_index += 1
        return d

    def sample_map(self, pi, batch_size):
        """``batch_size`` index pairs from the plan ``pi`` (one draw of the counter)."""
        return sample_plan(pi, batch_size, seed=self.seed, draw_index=self._next_draw())

    def sample_plan(self, x0, x1):
        """``(x0[i], x1[j])`` for B pairs drawn from the plan between the batches."""
        i, j = self.sample_map(self.get_map(x0, x1), x0.shape[0])
        return x0[i], x1[j]

    def sample_plan_with_labels(self, x0, x1, y0=None, y1=None):
        """``(x0[i], x1[j], y0[i] | None, y1[j] | None)``."""
        i, j = self.sample_map(self.get_map(x0, x1), x0.shape[0])
        return x0[i], x1[j], (y0[i] if y0 is not None else None), (y1[j] if y1 is not None else None)


def compute_ot_pairing_sinkhorn(source, target, reg=0.1, normalize_cost=True):
    """Upstream's ``compute_ot_pairing_vanilla``: the entropic plan with ``reg``, then for rows in order the largest plan entry among
    the unused targets (ties to the lowest).  Returns an int64 permutation on the inputs' device.  ``reg`` is relative to the largest
    cost here (``normalize_cost``): on raw squared distances of latents upstream's own call underflows to a zero kernel, and the
    log-domain solver would spend its 1000 iterations without converging."""
    return ot_plan_pairing(compute_ot_plan(source, target, reg=reg, normalize_cost=normalize_cost))


def compute_ot_pairing(source, target, debug=False, method="greedy", reg=0.1, normalize_cost=True):
    """ot.py:80-84.  ``method``: "greedy" (upstream's matcher, the default), "exact", or "sinkhorn" (upstream's vanilla variant:
    the entropic plan with ``reg`` as a permutation, ``compute_ot_pairing_sinkhorn``; ``reg`` / ``normalize_cost`` matter to it alone)."""
    if method == "greedy":
        return compute_ot_pairing_approximate(source, target)
    if method == "exact":
        return compute_ot_pairing_exact(source, target)
    if method == "sinkhorn":
        if not source.is_cuda:
            # a ValueError, as before this method existed: a caller that probed for it with host tensors still learns that only the
            # device serves it (compute_ot_pairing_sinkhorn itself raises RuntimeError, like 'greedy' and 'exact')
            raise ValueError("compute_ot_pairing: method='sinkhorn' has no CPU path (nor have 'greedy' and 'exact'): pass device tensors")
        return compute_ot_pairing_sinkhorn(source, target, reg=reg, normalize_cost=normalize_cost)
    raise ValueError(f"compute_ot_pairing: method must be 'greedy', 'exact' or 'sinkhorn', got {method!r}")


def pairing_cost(source, target, perm=None):
    """mean_i |source_i - target_perm[i]|^2 as a 0-d device tensor (``perm=None``: the identity): the figure that shows in a training
    log whether the pairing shortens the couplings."""
    bsz = source.shape[0]
    s = source.reshape(bsz, -1).float()
    t = target.reshape(bsz, -1).float()
    if perm is not None:
        t = t[perm.to(t.device)]
    return (s - t).square().sum(1).mean()
