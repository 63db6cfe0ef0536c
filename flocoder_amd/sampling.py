"""ODE sampling: host-side mirror of ``flocoder/sampling.py`` (reference lines cited per function) plus the legacy
Euler sampler (``legacy/train_sd_flowers.py:50-67``) that BASELINE's "64-step Euler" refers to.

Same names, argument meaning and return values as the reference.  When ``model`` is a ``flocoder_amd.Unet`` on a
GPU the whole trajectory runs inside the library (one hipGraph replay per step, time grid on the device, no host
sync per velocity call -- SURVEY Q6); any other callable model goes through the same formulas with torch ops on
the model's own device.
"""
from __future__ import annotations

import gc
import random
from functools import partial
from typing import Optional

import torch

from .unet import Unet, is_ones_mask, require_gpu, validate_t_eval, validate_tol


def warp_time(t, dt=None, s=.5):
    """Parametric time warp, sampling.py:23-33.  ``dt`` is accepted for signature parity; the reference's
    derivative branch is never used and mis-parenthesised, so it is not offered here."""
    if s < 0 or s > 1.5:
        raise ValueError(f"s={s} is out of bounds.")
    if dt:
        raise NotImplementedError("warp_time(dt=...) is dead code upstream (operator-precedence bug, sampling.py:31-32)")
    return 4 * (1 - s) * t ** 3 + 6 * (s - 1) * t ** 2 + (3 - 2 * s) * t


def rk4_time_grid(n_steps: int, init_strength: Optional[float] = None, dtype=torch.float32) -> torch.Tensor:
    """The grid generate_latents_rk4 integrates on (sampling.py:102,108-111): warp_time(linspace(...)), computed with
    the same CPU torch ops as the reference so the values are bit-identical."""
    if init_strength is None:
        ts = torch.linspace(0, 1, n_steps, dtype=dtype)
    else:
        ts = torch.linspace(init_strength, 1.0, max(1, int(n_steps * (1.0 - init_strength))), dtype=dtype)
    return warp_time(ts)


def euler_time_grid(sample_N: int, eps: float = 1e-3) -> torch.Tensor:
    """t_i = i/N*(1-eps)+eps in Python floats, rounded to fp32 by ``ones * t`` (train_sd_flowers.py:59-61)."""
    return torch.tensor([i / sample_N * (1 - eps) + eps for i in range(sample_N)], dtype=torch.float64).to(torch.float32)


@torch.no_grad()
def rk4_step(f, y, t, dt, debug=False):
    """sampling.py:36-48 (generic-model path; the Unet path runs this inside the captured graph)."""
    k1 = f(y, t)
    tpdto2 = t + dt / 2
    k2 = f(y + dt * k1 / 2, tpdto2)
    k3 = f(y + dt * k2 / 2, tpdto2)
    k4 = f(y + dt * k3, t + dt)
    return y + (dt / 6) * (k1 + 2 * k2 + 2 * k3 + k4)


@torch.no_grad()
def v_func_cfg(model, cond, cfg_strength, t_vec_template, x, t, t_scale=999, debug=False):
    """sampling.py:50-76 without the three host syncs per call."""
    t_vec = t_vec_template.fill_(float(t))
    v = model(x, t_vec * t_scale, cond=cond)
    if cond and cond.get('class_cond') is not None and cfg_strength:
        cond_no_class = cond.copy()
        cond_no_class['class_cond'] = None
        v_no_class = model(x, t_vec * t_scale, cond=cond_no_class)
        v = v_no_class + cfg_strength * (v - v_no_class)
    return v


def _mask_flags(cond):
    mask = cond.get('mask_cond') if isinstance(cond, dict) else None
    return mask, is_ones_mask(mask)                   # once per call


def _conditioning(model, cond, x=None, no_cpu_path=True):
    """The native / host fork of every entry.  ``cond`` as the samplers take it (a cond dict, a class-id tensor as the legacy samplers,
    or None) -> ``(cond dict, class ids, mask, mask_is_ones)``.  The last three are what the integrators of a ``flocoder_amd.Unet`` take
    and are made for one only: the mask test is a host sync, so call this once per public call, where the native path is taken.  With
    ``x``, the tensor the native path would integrate, a ``flocoder_amd.Unet`` on the CPU raises here (``no_cpu_path``: which of the two
    wordings the entry has always used)."""
    if cond is not None and not isinstance(cond, dict):
        cond = {'class_cond': cond}
    if not isinstance(model, Unet):
        return cond, None, None, False
    if x is not None:
        require_gpu(x, no_cpu_path)
    return (cond, cond.get('class_cond') if cond else None) + _mask_flags(cond)


def _start(source, shape, device):
    """The fp32 contiguous tensor an integrator updates in place: a copy of ``source`` on ``device``, or noise of ``shape``."""
    x = source if source is not None else torch.randn(shape, device=device)
    return x.to(device=device, dtype=torch.float32).contiguous().clone()


def _start_and_grid(model, shape, source, init_latents, init_strength, n_steps, fallback=None):
    """Start and grid of the fixed-grid generators (sampling.py:95-111) -> ``(current_points, ts, effective n_steps, device, dtype)``:
    ``source`` or randn on the device and in the dtype of the model's parameters; with ``init_latents`` the blend
    ``(1 - s) source + s init_latents`` on ``rk4_time_grid(n_steps, s)`` and the reference's ``max(1, int(n_steps (1 - s)))`` bookkeeping.
    ``fallback`` is the tensor whose device and dtype serve for a model without parameters; without one such a model raises."""
    has_params = hasattr(model, "parameters") and any(True for _ in model.parameters())
    p0 = next(model.parameters()) if has_params or fallback is None else fallback
    device, dtype = p0.device, p0.dtype
    current_points = source if source is not None else torch.randn(shape, device=device, dtype=dtype)
    if init_latents is None:
        return current_points, rk4_time_grid(n_steps, dtype=dtype), n_steps, device, dtype
    current_points = (1 - init_strength) * current_points + init_strength * init_latents
    return current_points, rk4_time_grid(n_steps, init_strength, dtype=dtype), max(1, int(n_steps * (1.0 - init_strength))), device, dtype


def _velocity(model, cond, cfg_strength, bsz, device, dtype=None):
    """``v(x, t)`` of a model that is not integrated in the library: ``v_func_cfg`` over a time vector of its own."""
    return partial(v_func_cfg, model, cond, cfg_strength, torch.zeros(bsz, device=device, dtype=dtype))


def _nfe(nfev, per_sample):
    """``Unet.integrate_rk45``'s nfev -> the samplers' nfe: per sample the largest, the number of batch forwards made."""
    return int(nfev.max()) if per_sample else nfev


def _rk4_loop(v_func, x, ts, jitter_strength=None):
    """``rk4_step`` along ``ts`` for models that are not a ``flocoder_amd.Unet``; with ``jitter_strength`` generate_latents_rk4's
    random kicks (sampling.py:117-119)."""
    for i in range(len(ts) - 1):
        x = rk4_step(v_func, x, ts[i], ts[i + 1] - ts[i])
        if jitter_strength is not None and random.random() < 0.1 and jitter_strength > 0:
            x += torch.randn_like(x) * jitter_strength * (1 - ts[i])
    return x


@torch.no_grad()
def generate_latents_rk4(model, shape, n_steps=50, cond=None, cfg_strength=3.0, source=None, init_latents=None,
                         init_strength=0.0, jitter_strength=0, debug=False):
    """sampling.py:78-122.  Returns (latents, n_steps*4) -- the reference's nfe bookkeeping."""
    current_points, ts, n_steps, device, dtype = _start_and_grid(model, shape, source, init_latents, init_strength, n_steps)
    if init_latents is None:
        jitter_strength = 0

    if isinstance(model, Unet) and not jitter_strength:
        x = _start(current_points, None, device)
        if len(ts) > 1:
            _, cls, mask, ones = _conditioning(model, cond)
            model.integrate("rk4", x, ts, class_ids=cls, cfg_strength=cfg_strength or 0.0, mask=mask, mask_is_ones=ones)
        return x, n_steps * 4

    v_func = _velocity(model, cond, cfg_strength, shape[0], device, dtype)
    return _rk4_loop(v_func, current_points, ts.to(device), jitter_strength), n_steps * 4


@torch.no_grad()
def generate_latents_guided(model, shape, measurement, keep, n_steps=50, init_strength=0.2, init_latents=None, cond=None, cfg_strength=3.0,
                            source=None, sigma_y=0.05, gamma=1.0, jacobian="identity"):
    """Training-free inpainting / editing with any pretrained flow (``inpainting.algorithm3``, the reference's inpainting.py:92-130, for a
    diagonal measurement operator): ``generate_latents_rk4(..., init_latents=..., init_strength=...)`` -- the same start
    ``(1 - s) source + s init_latents`` (``init_latents`` defaults to ``measurement``), the same grid ``rk4_time_grid(n_steps, s)``, the
    same nfe bookkeeping -- with every stage velocity (after classifier-free guidance) corrected towards ``measurement = keep * x_1``:

        x1 = x + (1-t) v      w = keep (measurement - keep x1) / (r2 keep^2 + sigma_y^2)      r2 = (1-t)^2 / (t^2 + (1-t)^2)
        v <- v + gamma ((1-t)/t) g        g = w (jacobian="identity", upstream)  |  w + (1-t) (dv/dx)^T w (jacobian="exact")

    at the stage's own state x and time t.  ``keep`` holds the weights in [0, 1] of the measured elements (x's shape or ``[B,1,H,W]``); for
    inpainting ``measurement = keep * known_latents``.  ``init_strength <= 0`` raises ValueError (the grid would contain t = 0, where
    the correction is unbounded), and so does ``jacobian="exact"`` together with class ids and a non-zero ``cfg_strength`` (the exact
    term differentiates one forward, not the guided pair).  Returns ``(latents, nfe)``.

    A ``flocoder_amd.Unet`` runs the loop in the library (``Unet.integrate_guided``: the identity form replays the captured RK4 step with
    guided stage kernels; the exact form runs a training-form forward and the backward plan's data-gradient chain per evaluation, and
    leaves the model's plans as it found them); on the CPU it raises like the other integrators.  Any other callable takes the torch
    path: ``rk4_step`` over the corrected field, ``torch.autograd.grad`` for the exact term."""
    from .inpainting import guidance_weight
    if jacobian not in ("identity", "exact"):
        raise ValueError(f"jacobian={jacobian!r}: 'identity' or 'exact'")
    if init_strength is None or not init_strength > 0:
        raise ValueError(f"init_strength={init_strength} must be > 0: the grid would contain t = 0, where the correction (1-t)/t is unbounded")
    if sigma_y < 0:
        raise ValueError("sigma_y must be >= 0")
    if tuple(measurement.shape) != tuple(shape):
        raise ValueError(f"measurement must have shape {tuple(shape)}, got {tuple(measurement.shape)}")
    if tuple(keep.shape) not in (tuple(shape), (shape[0], 1) + tuple(shape[2:])):
        raise ValueError(f"keep must have shape {tuple(shape)} or [B,1,H,W], got {tuple(keep.shape)}")
    unet = isinstance(model, Unet)
    cond, cls, mask, ones = _conditioning(model, cond)
    if jacobian == "exact" and cfg_strength and cond and cond.get('class_cond') is not None:
        raise ValueError("jacobian='exact' takes no classifier-free guidance (pass cfg_strength=0): the exact term differentiates one "
                         "forward, not the guided pair")
    current_points, ts, n_steps, device, dtype = _start_and_grid(model, shape, source, measurement if init_latents is None else init_latents,
                                                                 init_strength, n_steps, fallback=measurement)
    nfe = n_steps * 4

    if unet:
        require_gpu(current_points)                  # on its own here: the refusal above needs the cond dict before the start exists
        x = _start(current_points, None, device)
        if len(ts) > 1:
            model.integrate_guided(x, ts, measurement, keep, sigma_y=sigma_y, gamma=gamma, jacobian=jacobian, class_ids=cls,
                                   cfg_strength=cfg_strength or 0.0, mask=mask, mask_is_ones=ones)
        return x, nfe

    ts = ts.to(device)
    y, a = measurement.to(device=device, dtype=dtype), keep.to(device=device, dtype=dtype)
    v_cfg, t_vec_template = _velocity(model, cond, cfg_strength, shape[0], device, dtype), torch.zeros(shape[0], device=device, dtype=dtype)

    def v_func(x, t):
        om = 1 - t
        if jacobian == "identity":
            v = v_cfg(x, t)
            g = guidance_weight(v, x, t, y, a, sigma_y)
        else:
            with torch.enable_grad():
                xr = x.detach().requires_grad_(True)
                vr = model(xr, t_vec_template.fill_(float(t)) * 999, cond=cond)
                w = guidance_weight(vr.detach(), x, t, y, a, sigma_y)
                q, = torch.autograd.grad(vr, xr, w)
            v = vr.detach()
            g = w + om * q
        return v + (gamma * om / t) * g

    return _rk4_loop(v_func, current_points, ts), nfe


def _counter_field(host_field, native_field, seed, index, sample_ids, shape, device, dtype):
    """A counter-based field of ``flocoder_amd.noise`` as a tensor ``[B, *shape[1:]]``, row b that of ``(seed, index, sample_ids[b])``:
    ``native_field(lib, out, seed, index, ids, B, per-sample size, stream)`` on a GPU device, the NumPy ``host_field`` on the CPU."""
    from . import _binding as B
    device = torch.device("cpu" if device is None else device)
    bsz, per = int(shape[0]), 1
    for d in shape[1:]:
        per *= int(d)
    if device.type != "cuda":
        ids = sample_ids.detach().cpu().numpy() if torch.is_tensor(sample_ids) else sample_ids
        return torch.from_numpy(host_field(seed, index, ids, per)).reshape(tuple(shape)).to(device=device, dtype=dtype)
    ids = torch.as_tensor(sample_ids, dtype=torch.int64).to(device).contiguous()
    out = torch.empty(tuple(shape), dtype=torch.float32, device=device)
    B.check(native_field(B.lib(), B.ptr(out), int(seed) & 0xffffffffffffffff, int(index), B.ptr(ids), bsz, per, B.current_stream(device)))
    return out.to(dtype)


def normal_field(seed, draw_index, sample_ids, shape, device=None, dtype=torch.float32):
    """The counter-based normal field of the stochastic samplers as a tensor ``[B, *shape[1:]]``: row b holds the normals of
    ``(seed, draw_index, sample_ids[b])`` (``flocoder_amd.noise``).  On a GPU device the library generates it (``fc_ode_normal_field``, fp32
    arithmetic); on the CPU ``noise.normal_field`` does (fp64 arithmetic, then rounded to ``dtype``)."""
    from . import noise as N
    return _counter_field(N.normal_field, lambda lib, *args: lib.fc_ode_normal_field(*args), seed, draw_index, sample_ids, shape, device, dtype)


def probe_field(seed, probe_index, sample_ids, shape, kind="rademacher", device=None, dtype=torch.float32):
    """The likelihood's counter-based probe field as a tensor ``[B, *shape[1:]]``: row b holds probe ``probe_index`` of
    ``(seed, sample_ids[b])`` (``flocoder_amd.noise.probe_field``): it depends on those and the position in the sample, never on the
    row or the batch size.  On a GPU device the library generates it (``fc_ode_probe_field``); on the CPU the NumPy form does."""
    from . import noise as N
    if kind not in N.PROBE_KINDS:
        raise ValueError(f"kind={kind!r}: 'rademacher' or 'gaussian'")
    return _counter_field(lambda *args: N.probe_field(*args, kind), lambda lib, out, *args: lib.fc_ode_probe_field(out, N.PROBE_KINDS[kind], *args),
                          seed, probe_index, sample_ids, shape, device, dtype)


_SDE_EVALS = {"euler_maruyama": 1, "heun": 2}


@torch.no_grad()
def generate_latents_sde(model, shape, n_steps=50, cond=None, cfg_strength=3.0, source=None, init_latents=None, init_strength=0.0,
                         sigma=1.0, method="euler_maruyama", seed=0, sample_ids=None, noise=None):
    """Stochastic sampling: the SDE with the marginals of the probability-flow ODE that ``generate_latents_rk4`` integrates.  On the
    linear path ``x_t = (1-t) x0 + t x1`` with ``x0 ~ N(0, I)`` the score is ``(t v - x)/(1-t)``, and with diffusion ``sigma^2 (1-t)``

        dx = b(x,t) dt + sigma sqrt(1-t) dW          b(x,t) = (1 + sigma^2 t / 2) v(x,t) - (sigma^2 / 2) x

    (``v`` after classifier-free guidance; finite on all of [0, 1]).  Start and grid are ``generate_latents_rk4``'s: ``source`` (or randn),
    with ``init_latents`` the blend ``(1 - s) source + s init_latents`` on ``rk4_time_grid(n_steps, s)`` -- SDEdit-style editing.  Interval i
    with ``h = t_{i+1} - t_i``, ``a = sigma sqrt(h (1 - (t_i + t_{i+1})/2))`` (the exact standard deviation of the noise integral) and
    ``xi ~ N(0, I)``:

        method="euler_maruyama"   x+ = x + h b(x,t_i) + a xi
        method="heun"             xp = x + h b(x,t_i) + a xi;   x+ = x + (h/2) (b(x,t_i) + b(xp,t_{i+1})) + a xi      (the same xi)

    ``sigma = 0`` is deterministic Euler / Heun on the grid.  The noise is reproducible and independent of batching: ``xi`` of interval i
    and row b is the counter-based normal field of ``(seed, i, sample_ids[b])`` (``flocoder_amd.noise``; ``sample_ids`` int64 ``[B]``,
    default ``arange(B)`` -- a sharded caller passes the global indices of its rows), or ``noise[i]`` when a tensor
    ``[len(ts) - 1, *shape]`` is supplied.  Returns ``(latents, nfe)`` with nfe the true number of evaluations, ``(len(ts) - 1)`` times 1
    or 2 (a guided pair counts once).

    A ``flocoder_amd.Unet`` runs the loop in the library (``Unet.integrate_sde``: captured intervals, the noise generated inside the
    update kernel); on the CPU it raises like the other integrators.  Any other callable takes the torch path with the same field
    (``fc_ode_normal_field`` for GPU tensors, the NumPy form on the CPU)."""
    if method not in _SDE_EVALS:
        raise ValueError(f"method={method!r}: 'euler_maruyama' or 'heun'")
    sigma = float(sigma)
    if not sigma >= 0:
        raise ValueError("sigma must be >= 0")
    current_points, ts, _, device, dtype = _start_and_grid(model, shape, source, init_latents, init_strength, n_steps,
                                                           fallback=source if source is not None else torch.zeros(()))
    n_int = len(ts) - 1
    if n_int < 1:
        raise ValueError(f"n_steps={n_steps}, init_strength={init_strength}: the grid needs at least two points (one interval)")
    nfe = n_int * _SDE_EVALS[method]
    bsz = int(shape[0])
    if sample_ids is not None:
        sample_ids = torch.as_tensor(sample_ids)
        if sample_ids.dtype != torch.int64 or tuple(sample_ids.shape) != (bsz,):
            raise ValueError("sample_ids must be an int64 tensor of shape [batch]")
    if noise is not None and tuple(noise.shape) != (n_int,) + tuple(shape):
        raise ValueError(f"noise must have shape {(n_int,) + tuple(shape)}, got {tuple(noise.shape)}")

    cond, cls, mask, ones = _conditioning(model, cond, current_points)
    if isinstance(model, Unet):
        x = _start(current_points, None, device)
        model.integrate_sde(x, ts, sigma=sigma, method=method, seed=seed, sample_ids=sample_ids,
                            noise=None if noise is None else noise.to(device), class_ids=cls, cfg_strength=cfg_strength or 0.0, mask=mask,
                            mask_is_ones=ones)
        return x, nfe

    x = current_points.to(device)
    ts = ts.to(device)
    ids = torch.arange(bsz, dtype=torch.int64) if sample_ids is None else sample_ids
    v_func = _velocity(model, cond, cfg_strength, bsz, device, dtype)
    s2 = 0.5 * sigma * sigma
    drift = lambda xx, t: (1 + s2 * t) * v_func(xx, t) - s2 * xx
    for i in range(n_int):
        t0, t1 = ts[i], ts[i + 1]
        h = t1 - t0
        a = sigma * torch.sqrt(h * (1 - (t0 + t1) / 2))
        xi = noise[i].to(device=device, dtype=x.dtype) if noise is not None else normal_field(seed, i, ids, shape, device, x.dtype)
        b0 = drift(x, t0)
        if method == "euler_maruyama":
            x = x + h * b0 + a * xi
        else:
            xp = x + h * b0 + a * xi
            x = x + (h / 2) * (b0 + drift(xp, t1)) + a * xi
    return x, nfe


@torch.no_grad()
def euler_sampler(model, shape, sample_N, device=None, cond=None, source=None, eps=1e-3, cfg_strength=0.0):
    """Legacy Euler sampler, train_sd_flowers.py:50-67: x += model(x, 999 t_i, cond)/N on the un-warped grid, nfe = N.
    ``cond`` is a class-id tensor as upstream (wrapped into the dict the live Unet needs) or a cond dict;
    ``source`` replaces the randn start for reproducible runs.  ``cfg_strength`` is an extension (upstream has no
    CFG here; 0 keeps upstream behaviour).  Returns (latents on `device`, nfe)."""
    p0 = next(model.parameters())
    device = p0.device if device is None else torch.device(device)
    x = _start(source, shape, device)
    ts = euler_time_grid(sample_N, eps)
    dt = 1.0 / sample_N
    cond, cls, mask, ones = _conditioning(model, cond)
    if isinstance(model, Unet):
        model.integrate("euler", x, ts, dt_euler=dt, class_ids=cls, cfg_strength=cfg_strength, mask=mask, mask_is_ones=ones)
        return x, sample_N
    for t in ts.tolist():
        t_vec = torch.ones(shape[0], device=device) * t
        x = x + model(x, t_vec * 999, cond) * dt
    return x, sample_N


def _reverse_grid(n_steps, dtype=torch.float32):
    if int(n_steps) < 2:
        raise ValueError(f"n_steps={n_steps}: the grid needs at least two points (one interval)")
    return rk4_time_grid(int(n_steps), dtype=dtype).flip(0)


def _check_ode_method(method):
    if method not in ("rk4", "rk45"):
        raise ValueError(f"method={method!r}: 'rk4' (the reversed RK4 grid) or 'rk45' (adaptive, scipy's solve_ivp semantics)")


def _host_rk45_groups(x, cond, per_sample):
    """The controller groups of a host-side adaptive solve: ``(row slice, cond of those rows)`` -- the batch, or one per sample."""
    if not per_sample:
        return [(slice(0, x.shape[0]), cond)]
    return [(slice(b, b + 1), {k: (v[b:b + 1] if torch.is_tensor(v) else v) for k, v in cond.items()} if cond else cond)
            for b in range(x.shape[0])]


def _host_rk45(who, x, cond, per_sample, solve):
    """The host-side adaptive solves of ``who`` for models that are not a ``flocoder_amd.Unet``: every controller group of ``x`` on its
    own.  ``solve(rows, x[rows], cond of those rows)`` builds the group's state, integrates it and scatters the result into the caller's
    outputs; it returns ``(nfev, None)``, or ``(None, the solver's message)`` where scipy would return ``success=False``.  Returns the
    largest nfev; failed solves raise RuntimeError with the message, per sample naming the samples."""
    nfevs, failed = [], []
    for rows, cond_g in _host_rk45_groups(x, cond, per_sample):
        nfev, message = solve(rows, x[rows], cond_g)
        if message is None:
            nfevs.append(int(nfev))
        else:
            failed.append(f"sample {rows.start}: {message}" if per_sample else str(message))
    if failed:
        raise RuntimeError(f"{who}: {len(failed)} of {x.shape[0]} samples failed; " + " ".join(failed) if per_sample else f"{who}: {failed[0]}")
    return max(nfevs)


def _solve_ivp_rk45(ode_func, span, y0, rtol, atol, t_eval=None):
    """The legacy ``solve_ivp(method="RK45")`` call over ``span`` -> ``(solution, y at the end of the span)``.  With ``t_eval`` scipy
    returns the requested times only (``solution.y`` are the frames), so the solver's own final state is taken from an event function
    that never fires: solve_ivp hands it every accepted ``(t, y)`` and changes nothing else, the steps and the final state are those of
    the call without ``t_eval``."""
    import numpy as np
    from scipy import integrate
    if t_eval is None:
        solution = integrate.solve_ivp(ode_func, span, y0, rtol=rtol, atol=atol, method="RK45")
        return solution, solution.y[:, -1]
    last = [np.asarray(y0)]

    def watch(t, y):
        last[0] = np.array(y)
        return 1.0

    solution = integrate.solve_ivp(ode_func, span, y0, rtol=rtol, atol=atol, method="RK45", t_eval=t_eval, events=watch)
    return solution, last[0]


def _invert_rk45_host(model, latents, cond, rtol, atol, per_sample):
    """``invert_latents(method="rk45")`` for any callable: the legacy adaptive solve from t = 1 to t = 0 in the latents' dtype, no
    guidance."""
    import numpy as np
    out = latents.detach().clone()

    def solve(rows, xg, cond_g):
        shape = tuple(xg.shape)
        v_func = _velocity(model, cond_g, 0.0, shape[0], xg.device, xg.dtype)

        def ode_func(t, y):
            xt = torch.from_numpy(np.asarray(y).reshape(shape)).to(device=xg.device, dtype=xg.dtype)
            return v_func(xt, t).detach().double().cpu().numpy().reshape((-1,))

        sol, y_end = _solve_ivp_rk45(ode_func, (1.0, 0.0), xg.detach().double().cpu().numpy().reshape((-1,)), rtol, atol)
        if not sol.success:
            return None, sol.message
        out[rows] = torch.from_numpy(y_end.reshape(shape).copy()).to(device=xg.device, dtype=xg.dtype)
        return sol.nfev, None

    return out, _host_rk45("invert_latents", latents, cond, per_sample, solve)


@torch.no_grad()
def invert_latents(model, latents, n_steps=50, cond=None, method="rk4", rtol=1e-5, atol=1e-5, per_sample=True):
    """Data -> noise: the probability-flow ODE from t = 1 back to t = 0 on ``rk4_time_grid(n_steps)`` REVERSED, with the RK4 step and
    without guidance -- the ``z`` that ``generate_latents_rk4(..., source=z, cfg_strength=0)`` maps back to ``latents`` up to the
    discretisation error of the two solves.  ``cond`` as the samplers (a cond dict, or class ids).  Returns ``(z, nfe)`` with nfe the
    true number of velocity evaluations, ``4 (n_steps - 1)`` -- not ``generate_latents_rk4``'s ``n_steps * 4`` bookkeeping.
    A ``flocoder_amd.Unet`` runs the captured inference path (``Unet.integrate`` takes a grid in either direction); any other callable
    goes through ``rk4_step`` on the latents' device.

    ``method="rk45"`` replaces the grid by the legacy adaptive solver run backwards: ``solve_ivp(method="RK45", rtol, atol)`` from
    t = 1 to t = 0 (``n_steps`` is ignored), one problem per sample with ``per_sample`` (default) or one over the batch; nfe is scipy's
    ``nfev`` (per sample: the largest).  A ``flocoder_amd.Unet`` runs it in the library (``Unet.integrate_rk45``), any other callable
    through scipy on the host in the latents' dtype."""
    _check_ode_method(method)
    rk45 = method == "rk45"
    if rk45:
        rtol, atol = validate_tol(rtol, atol)
    else:
        ts = _reverse_grid(n_steps, torch.float32 if isinstance(model, Unet) else latents.dtype)
        nfe = 4 * (len(ts) - 1)
    cond, cls, mask, ones = _conditioning(model, cond, latents, no_cpu_path=False)
    if isinstance(model, Unet):
        x = _start(latents, None, latents.device)
        if not rk45:
            model.integrate("rk4", x, ts, class_ids=cls, cfg_strength=0.0, mask=mask, mask_is_ones=ones)
            return x, nfe
        nfev, _, _ = model.integrate_rk45(x, 1.0, 0.0, rtol=rtol, atol=atol, class_ids=cls, cfg_strength=0.0, mask=mask, mask_is_ones=ones,
                                          per_sample=per_sample)
        return x, _nfe(nfev, per_sample)
    if rk45:
        return _invert_rk45_host(model, latents, cond, rtol, atol, per_sample)
    return _rk4_loop(_velocity(model, cond, 0.0, latents.shape[0], latents.device, latents.dtype), latents, ts.to(latents.device)), nfe


def _make_probe(probe, latents, generator):
    if torch.is_tensor(probe):
        if probe.shape != latents.shape:
            raise ValueError(f"probe must have the shape of latents {tuple(latents.shape)}, got {tuple(probe.shape)}")
        return probe.to(device=latents.device, dtype=latents.dtype).contiguous()
    if probe not in ("rademacher", "gaussian"):
        raise ValueError(f"probe={probe!r}: 'rademacher', 'gaussian' or a tensor of the latents' shape")
    gdev = generator.device if generator is not None else latents.device
    if probe == "gaussian":
        e = torch.randn(latents.shape, generator=generator, device=gdev, dtype=latents.dtype)
    else:
        e = torch.randint(0, 2, latents.shape, generator=generator, device=gdev).to(latents.dtype) * 2 - 1
    return e.to(latents.device).contiguous()


def _make_probes(probe, latents, generator, n_probes, probe_seed, sample_ids):
    """The probes of a ``log_likelihood`` call -> (eps, K): eps of the latents' shape for a plain single-probe call (K is None: today's
    call), else ``[K, *latents.shape]``."""
    from . import _binding as B
    n_probes = int(n_probes)
    if torch.is_tensor(probe) and probe.dim() == latents.dim() + 1:
        if probe.shape[1:] != latents.shape:
            raise ValueError(f"probe must have the shape of latents {tuple(latents.shape)} or [K, ...] of it, got {tuple(probe.shape)}")
        if n_probes not in (1, probe.shape[0]):
            raise ValueError(f"n_probes={n_probes} does not agree with the probe tensor's {probe.shape[0]} probes")
        if probe_seed is not None:
            raise ValueError("probe_seed draws the probes: pass a kind ('rademacher', 'gaussian'), not a tensor")
        k = int(probe.shape[0])
        if not 1 <= k <= B.FC_LL_MAX_PROBES:
            raise ValueError(f"n_probes={k} must lie in [1, {B.FC_LL_MAX_PROBES}] (the cap on probes per call)")
        return probe.to(device=latents.device, dtype=latents.dtype).contiguous(), k
    if not 1 <= n_probes <= B.FC_LL_MAX_PROBES:
        raise ValueError(f"n_probes={n_probes} must lie in [1, {B.FC_LL_MAX_PROBES}] (the cap on probes per call)")
    if probe_seed is not None:
        if generator is not None:
            raise ValueError("probe_seed and generator are two sources of the probes: pass one")
        if torch.is_tensor(probe):
            raise ValueError("probe_seed draws the probes: pass a kind ('rademacher', 'gaussian'), not a tensor")
        ids = torch.arange(latents.shape[0]) if sample_ids is None else torch.as_tensor(sample_ids, dtype=torch.int64).reshape(-1)
        if ids.numel() != latents.shape[0]:
            raise ValueError(f"sample_ids must name the {latents.shape[0]} samples, got {ids.numel()}")
        eps = torch.stack([probe_field(probe_seed, k, ids, latents.shape, probe, latents.device, latents.dtype) for k in range(n_probes)])
        return eps.contiguous(), n_probes
    if sample_ids is not None:
        raise ValueError("sample_ids index the counter-based probes: pass probe_seed")
    if n_probes == 1:
        return _make_probe(probe, latents, generator), None
    if torch.is_tensor(probe):
        raise ValueError(f"n_probes={n_probes} needs a [K, ...] probe tensor or a kind to draw from")
    return torch.stack([_make_probe(probe, latents, generator) for _ in range(n_probes)]).contiguous(), n_probes


def _probe_stats(a_probes, a=None):
    """(mean in probe order with one division, standard error of the mean around ``a`` or that mean) of ``a_probes`` [K, B] fp64"""
    k = a_probes.shape[0]
    mean = a_probes[0].clone()
    for i in range(1, k):
        mean = mean + a_probes[i]
    mean = mean / k
    centre = mean if a is None else a
    se = torch.sqrt(((a_probes - centre) ** 2).sum(dim=0) / (k * (k - 1))) if k > 1 else torch.full_like(mean, float("nan"))
    return mean, se


def log_likelihood(model, latents, n_steps=50, cond=None, probe="rademacher", generator=None, cfg_strength=None, method="rk4", rtol=1e-5,
                   atol=1e-5, per_sample=True, t_end=0.0, n_probes=1, probe_seed=None, sample_ids=None, return_info=False):
    """log p_1(latents) under the flow: the change of variables along the probability-flow ODE walked from t = 1 to t = 0 on
    ``rk4_time_grid(n_steps)`` reversed, with Hutchinson's estimate of the divergence.  Interval by interval (dt < 0), every RK4 stage j
    gives ``v_j = model(x_j, 999 t_j, cond)`` and ``d_j[b] = sum_i eps[b,i] ((dv_j/dx_j)^T eps)[b,i]`` (one VJP of the same forward);

        x <- x + (dt/6)(v1 + 2 v2 + 2 v3 + v4)              a <- a + (dt/6)(d1 + 2 d2 + 2 d3 + d4)      (a = 0 at t = 1)

    and with ``z`` = x at t = 0:  ``logp[b] = -|z_b|^2 / 2 - (D/2) ln 2pi + a[b]``, D = C*H*W (a is the integral of div v from 1 to 0,
    hence the plus sign).  Returns ``(logp, z, nfe)``: ``logp`` fp64 ``[B]`` on the latents' device, ``z`` like ``latents``, nfe = the true
    number of velocity evaluations ``4 (n_steps - 1)`` (not ``generate_latents_rk4``'s ``n_steps * 4`` bookkeeping).
    ``metrics.bits_per_dim(logp, D)`` turns it into bits per (latent) dimension.

    ``probe``: ``"rademacher"`` (default: +-1 entries, exact for a diagonal Jacobian), ``"gaussian"``, or a tensor of the latents' shape;
    ONE probe per call, the same for all stages.  The trajectory does not depend on it, so the mean over K probes is K calls averaged.
    ``generator`` seeds the drawn probes.  ``cond``: ``class_cond`` gives log p(x | class); ``mask_cond`` is carried as data, as the
    samplers do.  Classifier-free guidance is refused (``cfg_strength`` other than 0 / None raises ValueError): the guided field is not
    the flow of a density the model defines.

    A ``flocoder_amd.Unet`` on the GPU runs the whole loop in the library (``Unet.log_likelihood``: training-mode forward, the backward
    plan's data-gradient chain and one small kernel per evaluation; x in fp32, d_j and a in fp64); on the CPU it raises like the other
    integrators.  Any other callable takes the torch path below in the dtype of ``latents`` (fp64 latents give an fp64 solve; d_j and a
    are fp64 either way).  The model's ``training`` flag, its parameters' ``requires_grad`` and ``.grad`` are left as found, and so is the
    form of a ``flocoder_amd.Unet``'s launch plans: a model that samples (inference-form plans) gets them back before the call returns, so a
    sampler call after it gives the bits of a model that never computed a likelihood (``Unet.log_likelihood``'s ``restore_plan``; it
    costs a device synchronisation and two plan builds per call -- for many calls in a row use ``Unet.log_likelihood(...,
    restore_plan=False)`` and ``Unet.release_training_plan()``).

    ``method="rk45"`` puts the integration error under control instead of leaving it to ``n_steps`` (which is then ignored): the
    literature's likelihood computation, ``scipy.integrate.solve_ivp(method="RK45", rtol, atol)`` from t = 1 to ``t_end`` (default 0; any
    value in [0, 1)) on the concatenated state ``[x, a]`` with ``da/dt = d``, ``a = 0`` at t = 1 -- the divergence integral takes part in
    the error norm (n = unknowns of x + one per sample) with the scale ``atol + rtol max(|a|, |a_new|)``.  ``per_sample=True`` (default: a
    sample's likelihood is its own quantity) solves every sample as its own problem; ``per_sample=False`` solves one problem over the
    batch, as the literature's code does.  ``logp`` is then ``-|z|^2/2 - (D/2) ln 2pi + a`` with ``z = x(t_end)``; nfe is scipy's
    ``nfev`` (per sample: the largest).  A ``flocoder_amd.Unet`` runs the solve in the library (``Unet.log_likelihood_rk45``:
    controller on the device, x in fp64 with fp32 evaluations, a entirely fp64); any other callable goes through ``solve_ivp`` on the
    host with ``torch.autograd.grad`` per evaluation, in the dtype of ``latents``.  A failed solve raises RuntimeError.

    Several probes in ONE solve: ``n_probes=K`` (1 <= K <= 64), or ``probe`` a ``[K, *latents.shape]`` tensor (``n_probes`` must then
    agree or stay 1).  The trajectory does not depend on the probe, so every evaluation is one forward and K VJPs, and ``nfe`` -- the
    number of VELOCITY evaluations -- does not grow with K.  RK4 grid: every probe carries its own accumulator ``a_k`` (bit-equal to a
    single-probe call with that probe on the device) and ``a = (a_1 + ... + a_K) / K``.  RK45: the state stays ``[x, a]`` with
    ``da/dt`` the mean of the K estimates, so K copies of one probe reproduce the single-probe solve; the ``a_k`` are by-products summed
    over the accepted steps.  Drawn probes come from ``generator`` as before (K draws, the first the one a K = 1 call makes) or, with
    ``probe_seed`` set (``generator`` must then be None), from the counter-based field ``probe_field(probe_seed, k, sample_ids, ...)``
    (``sample_ids`` default ``arange(B)``): a sample's probes, hence its ``logp``, then depend on its id and not on its row or batch.
    ``return_info=True`` appends a dict ``{"logp_stderr", "a", "a_probes", "n_probes"}``: ``logp_stderr`` fp64 ``[B]`` =
    ``sqrt(sum_k (a_k - a)^2 / (K (K - 1)))`` (NaN for K = 1), the standard error of ``logp`` from the estimator's variance;
    ``metrics.bits_per_dim_stderr`` converts it."""
    _check_ode_method(method)
    if cfg_strength:
        raise ValueError("log_likelihood takes no classifier-free guidance: the guided field is not the flow of a density the model defines")
    unet, rk45 = isinstance(model, Unet), method == "rk45"
    if rk45:
        rtol, atol = validate_tol(rtol, atol)
        t_end = float(t_end)
        if not 0.0 <= t_end < 1.0:
            raise ValueError(f"t_end={t_end} must lie in [0, 1)")
    else:
        ts = _reverse_grid(n_steps, torch.float32 if unet else latents.dtype)
        nfe = 4 * (len(ts) - 1)
    cond, cls, mask, ones = _conditioning(model, cond, latents)
    eps, k = _make_probes(probe, latents.float() if unet else latents, generator, n_probes, probe_seed, sample_ids)
    a_probes = stderr = None                          # of the paths that do not compute them; the tail does, and only for return_info
    if unet:
        z = _start(latents, None, latents.device)
        if rk45:
            (nfev, _, _), a, logp, *extra = model.log_likelihood_rk45(z, eps, 1.0, t_end, rtol=rtol, atol=atol, per_sample=per_sample,
                                                                      class_ids=cls, mask=mask, mask_is_ones=ones)
            nfe = _nfe(nfev, per_sample)
        else:
            a, logp, *extra = model.log_likelihood(z, ts, eps, class_ids=cls, mask=mask, mask_is_ones=ones)
        if k:
            a_probes, stderr = extra
    elif rk45:
        logp, z, a, nfe, a_probes = _log_likelihood_rk45_host(model, latents, cond, eps, rtol, atol, per_sample, t_end)
    else:
        logp, z, a, a_probes = _log_likelihood_torch(model, latents, ts.to(latents.device), cond, eps)
    if not return_info:
        return logp, z, nfe
    if a_probes is None:                              # the library's single-probe entries: the one probe's integral is ``a``
        a_probes, stderr = a[None].clone(), torch.full_like(a, float("nan"))
    elif stderr is None:                              # the host paths (on the RK4 grid ``a`` is the probes' mean itself)
        stderr = _probe_stats(a_probes, a)[1]
    return logp, z, nfe, {"logp_stderr": stderr, "a": a, "a_probes": a_probes, "n_probes": k or 1}


def _hutchinson(model, x, t, cond, eps_k, e64, t_scale):
    """One evaluation of the host likelihoods: ``v = model(x, t_scale t, cond)`` and ``torch.autograd.grad(v, x, eps_k)`` per probe (the
    graph is retained for all but the last) -> ``(v, d)``, ``d[k, b] = sum_i eps_k[b,i] ((dv/dx)^T eps_k)[b,i]`` in fp64 (``e64``: the
    probes as fp64)."""
    n_k = eps_k.shape[0]
    with torch.enable_grad():
        xr = x.detach().requires_grad_(True)
        t_vec = torch.full((x.shape[0],), float(t), device=x.device, dtype=x.dtype)
        v = model(xr, t_vec * t_scale, cond=cond)
        gs = [torch.autograd.grad(v, xr, eps_k[k], retain_graph=k + 1 < n_k)[0] for k in range(n_k)]
    return v.detach(), torch.stack([(e64[k] * gs[k].double()).flatten(1).sum(dim=1) for k in range(n_k)])


def _logp(z, a):
    """``-|z_b|^2 / 2 - (D/2) ln 2pi + a[b]`` in fp64"""
    import math
    return -0.5 * z.double().flatten(1).pow(2).sum(dim=1) - 0.5 * z[0].numel() * math.log(2 * math.pi) + a


def _log_likelihood_torch(model, latents, ts, cond, eps, t_scale=999):
    """The loop of ``log_likelihood`` with torch ops: one forward per stage and one VJP per probe (``_hutchinson``; ``eps`` of the
    latents' shape, or ``[K, ...]``).  Every probe carries its own accumulator; ``a`` is their mean in probe order (one probe: its
    accumulator).  Returns (logp, z, a, a_probes [K, B])."""
    eps_k = eps if eps.dim() == latents.dim() + 1 else eps[None]
    n_k, e64 = eps_k.shape[0], eps_k.double()

    def stage(x, t):
        return _hutchinson(model, x, t, cond, eps_k, e64, t_scale)

    x = latents.detach()
    a_probes = torch.zeros(n_k, latents.shape[0], dtype=torch.float64, device=x.device)
    for i in range(len(ts) - 1):
        t, dt = ts[i], ts[i + 1] - ts[i]
        tpdto2 = t + dt / 2
        k1, d1 = stage(x, t)
        k2, d2 = stage(x + dt * k1 / 2, tpdto2)
        k3, d3 = stage(x + dt * k2 / 2, tpdto2)
        k4, d4 = stage(x + dt * k3, t + dt)
        x = x + (dt / 6) * (k1 + 2 * k2 + 2 * k3 + k4)
        a_probes = a_probes + (dt.double() / 6) * (d1 + 2 * d2 + 2 * d3 + d4)
    a = _probe_stats(a_probes)[0] if n_k > 1 else a_probes[0]
    return _logp(x, a), x, a, a_probes


def _log_likelihood_rk45_host(model, latents, cond, eps, rtol, atol, per_sample, t_end=0.0, t_scale=999):
    """``log_likelihood(method="rk45")`` for any callable: ``solve_ivp(method="RK45")`` from 1 to ``t_end`` on the concatenated vector
    ``[x, a]`` of every controller group (the batch, or each sample), one forward and one VJP per probe and evaluation (``_hutchinson``;
    ``eps`` of the latents' shape, or ``[K, ...]``); ``da/dt`` is the probes' mean, summed in probe order with one division.

    ``solve_ivp`` is ``RK45(...)`` stepped until it finishes; the solver object is driven directly here -- same steps, same bits -- so
    that the per-probe integrals can be recovered: after a successful ``step()`` the accepted attempt is the six evaluations made last
    plus the first-same-as-last one carried over, and ``a_k += h sum_s B_s d_{s,k}`` over them.  Returns (logp, z, a, nfe,
    a_probes [K, B])."""
    import numpy as np
    from scipy.integrate import RK45
    eps_k = eps if eps.dim() == latents.dim() + 1 else eps[None]
    n_k = eps_k.shape[0]
    z, a = latents.detach().clone(), torch.zeros(latents.shape[0], dtype=torch.float64, device=latents.device)
    a_probes = torch.zeros(n_k, latents.shape[0], dtype=torch.float64, device=latents.device)

    def solve(rows, xg, cond_g):
        eg, e64 = eps_k[:, rows], eps_k[:, rows].double()
        shape, n = tuple(xg.shape), xg.numel()
        evals = []                                        # d_{.,k} of every evaluation, in the order made: [K, rows] each

        def ode_func(t, y):
            xt = torch.from_numpy(np.ascontiguousarray(y[:n]).reshape(shape)).to(device=xg.device, dtype=xg.dtype)
            v, dk = _hutchinson(model, xt, t, cond_g, eg, e64, t_scale)
            evals.append(dk.cpu().numpy())
            d = dk[0]
            if n_k > 1:
                for k in range(1, n_k):
                    d = d + dk[k]
                d = d / n_k
            return np.concatenate([v.double().cpu().numpy().reshape(-1), d.cpu().numpy()])

        y0 = np.concatenate([xg.detach().double().cpu().numpy().reshape(-1), np.zeros(shape[0])])
        solver = RK45(ode_func, 1.0, y0, t_end, rtol=rtol, atol=atol)      # f(t0, y0) and select_initial_step's second evaluation
        carried, ak, message = evals[0], np.zeros((n_k, shape[0])), None
        while solver.status == "running":
            message = solver.step()
            if solver.status == "failed":
                return None, message
            ks = [carried] + evals[-6:-1]                 # K0..K5 of the accepted attempt; evals[-1] is f(t + h, y_new), the next K0
            acc = ks[0] * solver.B[0]
            for s_ in range(1, 6):
                acc = acc + ks[s_] * solver.B[s_]
            ak = ak + (solver.t - solver.t_old) * acc
            carried = evals[-1]
            del evals[:-1]
        z[rows] = torch.from_numpy(solver.y[:n].reshape(shape).copy()).to(device=xg.device, dtype=xg.dtype)
        a[rows] = torch.from_numpy(solver.y[n:].copy()).to(a.device)
        a_probes[:, rows] = torch.from_numpy(ak).to(a.device)
        return solver.nfev, None

    nfe = _host_rk45("log_likelihood", latents, cond, per_sample, solve)
    return _logp(z, a), z, a, nfe, a_probes


def _host_frames(solution, n_eval, shape, device):
    """``solution.y`` of a solve with ``t_eval`` ([unknowns, F]; an empty list for no times) -> fp32 ``[F, *shape]``."""
    import numpy as np
    if n_eval == 0:
        return torch.empty((0,) + tuple(shape), dtype=torch.float32, device=device)
    y = np.asarray(solution.y, dtype=np.float64).reshape(-1, n_eval)
    return torch.tensor(y.T.copy()).reshape((n_eval,) + tuple(shape)).type(torch.float32).to(device)


@torch.no_grad()
def rk45_sampler(model, shape, device=None, cond=None, source=None, eps=1e-3, rtol=1e-5, atol=1e-5, cfg_strength=0.0, per_sample=False,
                 t_eval=None):
    """Legacy adaptive sampler, train_sd_flowers.py:78-107: ``scipy.integrate.solve_ivp(method="RK45")`` over ``(eps, 1)`` on
    ``model(float32(x), float32(t) * 999, cond)``; returns ``(latents, nfe)`` with nfe = scipy's ``solution.nfev``.  ``cond`` is a class-id
    tensor as upstream or a cond dict; ``source`` replaces the randn start; ``cfg_strength`` is an extension (0 keeps upstream behaviour;
    a guided pair counts as one evaluation).  The batch is ONE system of B*C*H*W unknowns with one step size and one error norm, as
    upstream, so a sample's trajectory depends on the rest of its batch.  A ``flocoder_amd.Unet`` runs the whole solve in the library
    (Unet.integrate_rk45: stages, error norm and step controller on the device); any other model takes the legacy host path through
    numpy.  Where scipy would return ``success=False`` (step size below the spacing of t) this raises RuntimeError -- the legacy code
    silently used the last state -- and no frames are returned either.

    ``per_sample=True`` is an extension: every sample is its own solve_ivp problem over its C*H*W unknowns (own initial step, error
    norm, step size, counters), so a sample's result depends only on its own source, class id and mask, not on how samples are
    grouped into batches.  nfe is then the largest per-sample nfev: the number of batch forwards the device path makes.  A failing
    sample raises RuntimeError naming it.

    ``t_eval`` (a sequence, array or tensor of times in ``[eps, 1]``, increasing) is solve_ivp's: the solver steps exactly as it would
    have, and every accepted step evaluates its quartic interpolant at the requested times inside it (per sample: each sample's own
    steps).  Returns ``(latents, nfe, frames)`` with ``frames`` fp32 ``[F, B, C, H, W]``; ``latents`` and ``nfe`` are bit for bit those
    of the call without ``t_eval``.  ``latents`` is still the solver's state at t = 1 -- unlike ``solve_ivp(..., t_eval=...).y[:, -1]``,
    which is the LAST REQUESTED time (at ``t_eval[-1] == 1`` the interpolant there: equal to ``latents`` to rounding, not in bits).
    Bad times raise solve_ivp's ValueErrors before any work."""
    rtol, atol = validate_tol(rtol, atol)
    te = None if t_eval is None else validate_t_eval(t_eval, eps, 1)
    p0 = next(model.parameters())
    device = p0.device if device is None else torch.device(device)
    x = _start(source, shape, device)
    cond, cls, mask, ones = _conditioning(model, cond)
    if isinstance(model, Unet):
        nfev, *rest = model.integrate_rk45(x, eps, 1.0, rtol=rtol, atol=atol, class_ids=cls, cfg_strength=cfg_strength or 0.0, mask=mask,
                                           mask_is_ones=ones, per_sample=per_sample, t_eval=te)
        return (x, _nfe(nfev, per_sample)) if te is None else (x, _nfe(nfev, per_sample), rest[2])

    # any other model: the legacy host path through numpy in fp32, the batch as one solve_ivp problem or (per_sample) the model called on
    # every sample alone (its class id and mask row)
    import numpy as np
    out = x.clone()
    frames = None if te is None else torch.empty((len(te),) + tuple(x.shape), dtype=torch.float32, device=device)

    def solve(rows, xg, cond_g):
        shape = tuple(xg.shape)
        v_func = _velocity(model, cond_g, cfg_strength, shape[0], device)

        def ode_func(t, y):
            xt = torch.from_numpy(np.asarray(y).reshape(shape)).to(device).type(torch.float32)
            return v_func(xt, t).detach().cpu().numpy().reshape((-1,))

        solution, y1 = _solve_ivp_rk45(ode_func, (eps, 1), xg.detach().cpu().numpy().reshape((-1,)), rtol, atol, te)
        if not solution.success:
            return None, solution.message
        out[rows] = torch.tensor(y1).reshape(shape).type(torch.float32).to(device)
        if te is not None:
            frames[:, rows] = _host_frames(solution, len(te), shape, device)
        return solution.nfev, None

    nfe = _host_rk45("rk45_sampler", x, cond, per_sample, solve)
    return (out, nfe) if te is None else (out, nfe, frames)


@torch.no_grad()
def generate_latents_rk45(model, shape, device=None, cond=None, cfg_strength=3.0, source=None, rtol=1e-5, atol=1e-5, per_sample=False,
                          t_eval=None):
    """The function sampling.py:142-143 dispatches to (undefined upstream): the legacy RK45 sampler over (1e-3, 1), no time warp, with
    classifier-free guidance as generate_latents_rk4 applies it.  ``per_sample=True`` solves every sample on its own (rk45_sampler).
    Returns (latents, nfe); with ``t_eval`` (times in [1e-3, 1], see rk45_sampler) ``(latents, nfe, frames)``: the trajectory at those
    times as ``[F, B, C, H, W]``, e.g. for ``decode_latents(codec, frames.flatten(0, 1))``; ``latents`` stays the state at t = 1."""
    return rk45_sampler(model, shape, device=device, cond=cond, source=source, eps=1e-3, rtol=rtol, atol=atol, cfg_strength=cfg_strength,
                        per_sample=per_sample, t_eval=t_eval)


@torch.no_grad()
def generate_latents(model, shape, method='rk4', n_steps=50, cond=None, cfg_strength=3.0, device=None, source=None,
                     init_latents=None, init_strength=0.0, debug=False, **sde_kw):
    """sampling.py:128-146.  'rk45' selects generate_latents_rk45 (undefined upstream; built here from the legacy RK45
    sampler); 'rk45_per_sample' selects it with one solve per sample (an extension); 'euler' selects the legacy sampler; 'sde' /
    'sde_heun' select generate_latents_sde with the Euler-Maruyama / Heun step (an extension; its keywords ``sigma``, ``seed``,
    ``sample_ids``, ``noise`` pass through and are refused for every other method)."""
    if method in ("sde", "sde_heun"):
        return generate_latents_sde(model, shape, n_steps, cond, cfg_strength, source=source, init_latents=init_latents,
                                    init_strength=init_strength, method="heun" if method == "sde_heun" else "euler_maruyama", **sde_kw)
    if sde_kw:
        raise TypeError(f"generate_latents(method={method!r}) takes no {sorted(sde_kw)}")
    if method in ("rk45", "rk45_per_sample"):
        if init_latents is not None:
            raise ValueError(f"init_latents is not defined for method={method!r} (upstream has no such integration)")
        return generate_latents_rk45(model, shape, device, cond, cfg_strength, source=source, per_sample=method == "rk45_per_sample")
    if method == "euler":
        # (the legacy sampler has no guidance upstream: generate_latents keeps that; sample_many forwards its cfg_strength itself)
        return euler_sampler(model, shape, n_steps, device=device, cond=cond, source=source)
    return generate_latents_rk4(model, shape, n_steps, cond, cfg_strength, source=source, init_latents=init_latents,
                                init_strength=init_strength)


def _decode_latents(codec, latents, is_midi=False, keep_gray=False, device=None, debug=False):
    """sampling.py:150-166."""
    if device is None:
        try:
            device = next(codec.parameters()).device
        except Exception:
            device = latents.device
    decoded = codec.decode(latents.to(device))
    if is_midi:
        from .metrics import g2rgb
        return g2rgb(decoded, keep_gray=keep_gray)
    return decoded


def decode_latents(codec, latents, is_midi=False, keep_gray=False, device=None, chunk_size=128, debug=False):
    """sampling.py:169-183; chunks stay on the device (upstream bounces every chunk through the CPU)."""
    chunks = [_decode_latents(codec, latents[i:i + chunk_size], is_midi=is_midi, keep_gray=keep_gray, device=device)
              for i in range(0, latents.shape[0], chunk_size)]
    return torch.cat(chunks, dim=0).to(latents.device)


@torch.no_grad()
def sampler(model, codec, method='rk4', batch_size=256, n_steps=100, cond=None, n_classes=0, latent_shape=(4, 16, 16),
            cfg_strength=3.0, is_midi=False, keep_gray=False, device=None, source=None, init_image=None, init_strength=0.0,
            debug=False, **sde_kw):
    """sampling.py:186-229: integrate, then decode.  Returns (pred_latents, decoded_pred, nfe).  ``method`` as ``generate_latents``,
    'sde' / 'sde_heun' included (their keywords pass through).
    Tolerates parameter-less codecs and cond=None, which crash upstream."""
    if device is None:
        device = next(model.parameters()).device
    try:
        codec_device = next(codec.parameters()).device
        assert device == codec_device, f"sampler, device mismatch: device = {device}, but  codec_device {codec_device}"
    except StopIteration:
        pass
    cond = {} if cond is None else cond

    init_latents = None
    if init_image is not None:
        if isinstance(init_image, str):
            raise NameError("init_image as a path is dead upstream (Image is never imported, sampling.py:204)")
        init_tensor = init_image if torch.is_tensor(init_image) else _to_tensor(init_image)
        if init_tensor.dim() == 3:
            init_tensor = init_tensor.unsqueeze(0)
        init_latents = codec.encode(init_tensor.to(device))
        if init_latents.shape[0] == 1 and batch_size > 1:
            init_latents = init_latents.repeat(batch_size, 1, 1, 1)

    shape = (batch_size,) + tuple(latent_shape)
    if source is not None:
        source = source[:batch_size]
    if cond.get('class_cond') is None and n_classes > 0:
        cond['class_cond'] = torch.randint(n_classes, (10,)).repeat(batch_size // 10).to(device)
    elif cond.get('class_cond') is not None:
        cond['class_cond'] = cond['class_cond'][:batch_size]
    if cond.get('mask_cond') is not None:
        cond['mask_cond'] = cond['mask_cond'][:batch_size]

    pred_latents, nfe = generate_latents(model, shape, method, n_steps, cond, cfg_strength, device=device, source=source,
                                         init_latents=init_latents, init_strength=init_strength, **sde_kw)
    decoded_pred = decode_latents(codec, pred_latents, is_midi, keep_gray, device=device)
    return pred_latents, decoded_pred, nfe


@torch.no_grad()
def evaluate_model(model, codec, epoch, target_latents, cond=None, batch_size=256, n_classes=0, latent_shape=(4, 16, 16), method='rk4',
                   n_steps=None, is_midi=False, keep_gray=False, tag="", cb_tracker=None, cfg_strength=3.0, output_dir="./",
                   use_wandb=False, pre_encoded=True, source=None, mask_pixels=None, debug=False, *, return_images=False,
                   inception=None, init_image=None, init_strength=0.0, prdc_k=None, frechet=False, kid=False):
    """sampling.py:233-322: one epoch's evaluation -- sample, decode, score -- in upstream's order of work: ``model.eval()`` /
    ``codec.eval()``; ``sampler`` with ``n_classes=0`` and the latent shape of ``target_latents``; decode ``target_latents[:batch_size]``;
    ``compute_sample_metrics``; when the codec has a ``vq`` and ``cb_tracker`` is given, the indices of all of ``target_latents`` go to
    the tracker as "val" and those of the generated latents as "gen" (``cb_tracker.analyze(codec, epoch)`` then gives the statistics
    upstream sends to wandb); ``model.train()``; the metrics dictionary is returned.  Everything stays on the device until the
    dictionary's numbers are read.  It composes ``sampler``, ``decode_latents``, ``metrics.compute_sample_metrics`` and
    ``metrics.calc_note_metrics`` and adds no sampler logic of its own.

    Differences from upstream:
    * ``n_steps=None`` means 100, which is what upstream effectively runs: it never forwards its own ``n_steps`` to ``sampler``, whose
      default is 100.  A value given here IS forwarded.
    * ``use_wandb`` defaults to False and True raises: wandb logging and the plots of the codebook analysis are out of scope.
    * No image grids are written (``tag`` and ``output_dir`` are accepted and unused).  ``return_images=True`` returns
      ``(metrics, images)`` with upstream's image dictionary instead: pred / target latents and decodes, the source and its decode when
      ``source`` is given, ``mask_latents`` / ``mask_pixels`` when they are.
    * With ``is_midi=True`` the note metrics of ``decoded_pred`` against ``decoded_target`` (as ``compute_sample_metrics`` leaves them:
      it rescales ``decoded_pred`` to the target's range in place, as upstream) are added under ``note/<key>``; if ``mask_pixels``
      [B,1,H,W] is given as well, the same metrics restricted to the pixels that were masked (mask > 0.5) under ``note_masked/<key>``.
    * Keyword-only ``inception`` goes to ``compute_sample_metrics`` (FID needs a local feature extractor), ``init_image`` /
      ``init_strength`` to ``sampler``, ``prdc_k`` (an integer) to ``compute_sample_metrics``: it adds ``prdc/precision``, ``prdc/recall``,
      ``prdc/density`` and ``prdc/coverage`` of the generated latents against ``target_latents``; with None the dictionary is unchanged.
      ``frechet`` / ``kid`` go there too and add ``frechet``, ``frechet_px`` / ``kid``, ``kid_px`` (``flocoder_amd.distances``) on the sets
      that ``sinkhorn`` / ``sinkhorn_px`` compare; with False the dictionary is unchanged.
    * ``gc.collect()`` / ``torch.cuda.empty_cache()`` are not called: nothing here bounces through the host that they would free."""
    if use_wandb:
        raise NotImplementedError("evaluate_model: wandb logging and image grids are out of scope; log the returned dictionary")
    from . import metrics as M
    model.eval(), codec.eval()
    latent_shape = target_latents.shape[-3:]
    pred_latents, decoded_pred, nfe = sampler(model, codec, method=method, batch_size=batch_size, n_steps=100 if n_steps is None else n_steps,
                                              cond=cond, n_classes=0, latent_shape=latent_shape, cfg_strength=cfg_strength, is_midi=is_midi,
                                              keep_gray=keep_gray, source=source, init_image=init_image, init_strength=init_strength)
    decoded_target = decode_latents(codec, target_latents[:batch_size], is_midi, keep_gray)
    metrics = M.compute_sample_metrics(pred_latents, target_latents, decoded_pred, decoded_target, inception=inception, prdc_k=prdc_k,
                                       frechet=frechet, kid=kid)

    if hasattr(codec, 'vq') and cb_tracker is not None:
        for name, lat in (("val", target_latents), ("gen", pred_latents)):
            if hasattr(codec.vq, "quantize_nchw"):                      # same vectors in the same order, without the two transposes
                _, indices, _ = codec.vq.quantize_nchw(lat)
            else:
                _, indices, _ = codec.vq(lat.permute(0, 2, 3, 1).reshape(-1, lat.shape[1]))
            cb_tracker.update_counts(name, indices.reshape(-1, indices.shape[-1]))

    if mask_pixels is not None:
        mask_pixels = mask_pixels[:batch_size].float()
    if is_midi:
        metrics.update({f'note/{k}': v for k, v in M.calc_note_metrics(decoded_pred, decoded_target, keep_gray=keep_gray, images=False)[0].items()})
        if mask_pixels is not None:
            region = mask_pixels if mask_pixels.dim() == 4 else mask_pixels.unsqueeze(1)
            masked = M.calc_note_metrics(decoded_pred, decoded_target, keep_gray=keep_gray, region=region, images=False)[0]
            metrics.update({f'note_masked/{k}': v for k, v in masked.items()})

    images = None
    if return_images:
        images = {'pred_latents': pred_latents, 'target_latents': target_latents, 'decoded_pred': decoded_pred, 'decoded_target': decoded_target}
        if source is not None:
            images.update({'source_latents': source[:batch_size], 'decoded_source': decode_latents(codec, source[:batch_size], is_midi, keep_gray)})
        if cond and isinstance(cond, dict) and cond.get('mask_cond') is not None:
            images['mask_latents'] = cond['mask_cond'][:batch_size]
        if mask_pixels is not None:
            images['mask_pixels'] = mask_pixels
    model.train()
    return (metrics, images) if return_images else metrics


@torch.no_grad()
def sample_many(model, shape, batches, method="euler", n_steps=64, cfg_strength=0.0, in_flight=2):
    """Throughput mode for callers that generate MANY batches (the 50 k samples of an FID run, evaluate_model / generate_samples loops around
    sampling.py:186-229): ``batches`` is a sequence of ``(cond, source)`` pairs, one per call of ``generate_latents`` the reference would
    make; up to ``in_flight`` of them run at the same time, each on its own stream and its own replica of ``model`` (own activation arena and
    captured graphs, weights copied once).  Trajectories are independent, so results equal the one-at-a-time calls; one trajectory is a chain
    of ~4500 dependent launches with the chip mostly waiting on launch-to-launch latency, and a second chain fills those gaps: measured
    955-975 samples/s against 782-789 for one batch of 64 at a time (tools/inflight_sweep.py, under AMD_DIRECT_DISPATCH=0 --
    ``flocoder_amd.apply_runtime_defaults("sampling")``).  The replicas run the plan without cross-workgroup waits (``set_shared_device``).
    ``method="rk45_per_sample"`` solves every sample on its own, so its results equal the one-at-a-time calls however the samples are
    grouped; but each such call waits on the host behind every attempt until its solve ends, so batches in flight do not overlap and
    ``in_flight`` buys no throughput there.  (The batch-coupled "rk45" couples the samples of a batch and is not meant for this mode.)
    Returns the list of latents in the order of ``batches``."""
    if not isinstance(model, Unet):
        raise TypeError("sample_many drives flocoder_amd.Unet replicas")
    dev = next(model.parameters()).device
    in_flight = max(1, int(in_flight))
    reps = getattr(model, "_replicas", None) or []
    while len(reps) < in_flight - 1:
        reps.append(model.replica())
    model._replicas = reps
    models = [model] + reps[: in_flight - 1]
    was = [m._shared for m in models]
    for m in models:
        m.set_shared_device(True if in_flight > 1 else None)
    streams = [torch.cuda.Stream(dev) for _ in models]
    cur = torch.cuda.current_stream(dev)
    outs = []
    try:
        for st in streams:
            st.wait_stream(cur)
        for i, (cond, source) in enumerate(batches):
            k = i % len(models)
            with torch.cuda.stream(streams[k]):
                if method == "euler":       # generate_latents' euler branch has no guidance (as upstream); euler_sampler's extension does
                    lat, _ = euler_sampler(models[k], shape, n_steps, cond=cond, source=source, cfg_strength=cfg_strength)
                else:
                    lat, _ = generate_latents(models[k], shape, method=method, n_steps=n_steps, cond=cond, cfg_strength=cfg_strength, source=source)
                outs.append(lat)
        for st in streams:
            cur.wait_stream(st)
        for m in models:
            m.check_errors(synchronize=False)
    finally:
        for m, w in zip(models, was):
            m.set_shared_device(w)
    return outs


def _to_tensor(img):
    """PIL image -> float CHW in [0,1] (torchvision.transforms.ToTensor, absent here)."""
    import numpy as np
    a = np.asarray(img)
    if a.ndim == 2:
        a = a[:, :, None]
    t = torch.from_numpy(a.copy()).permute(2, 0, 1)
    return t.float() / 255.0 if t.dtype == torch.uint8 else t.float()
