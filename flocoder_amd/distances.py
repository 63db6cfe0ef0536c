"""Frechet and kernel (KID) distances between sample sets, on the device (csrc/frechet.hip; no upstream counterpart).

With A = (X - mx) / sqrt(N1 - 1) and B = (Y - my) / sqrt(N2 - 1) the covariances are S1 = A^T A and S2 = B^T B, the non-zero eigenvalues of
S1 S2 are those of (A B^T)(A B^T)^T, and so

    FD = |mx - my|^2 + tr S1 + tr S2 - 2 ||A B^T||_*          (nuclear norm of an N1 x N2 matrix)

exactly: no D x D matrix is formed, D is the inner extent of one fp64 Gram product (fp32 rows, centred in fp64 on load, fp64 matrix
pipe).  The singular values come from a one-sided Jacobi iteration on the rows of that Gram (the smaller set first), which keeps its
relative accuracy on the rank-deficient matrices that N < D gives.  DESIGN.md section 4 "Set distances" has the error bound.

- ``gram(a, b, center=False)`` -- the fp64 ``[N1, N2]`` Gram of two sets, optionally of the centred sets;
- ``singular_values(m)`` -- ``(svals, info)`` of an fp64 ``[n, r]`` device matrix (n <= 4096), descending; ``info`` has ``sweeps``,
  ``converged`` and ``nuclear`` (the sum, a 0-d device tensor);
- ``frechet_distance_sets(real, fake, return_info=False)`` -- FD as a Python float; with ``return_info`` also a dict (``sweeps``,
  ``converged``, ``launches``, ``mean_term``, ``trace_real``, ``trace_fake``, ``nuclear``, ``svals``);
- ``kernel_distance(real, fake)`` -- the unbiased MMD^2 with k(x, y) = (x.y / D + 1)^3 over ALL pairs (no random subsets).
- ``FrechetMoments`` and ``frechet_distance_moments(a, b, return_info=False)`` -- the moment form for N >> D, below.

Samples of any shape are flattened per row.  2 <= N; min(N1, N2) <= 4096 and max(N1, N2) <= 16384 for the Frechet distance, N <= 16384
for the kernel distance.  A solve that does not converge (a non-finite input, or 30 sweeps) raises RuntimeError.  Sums run in a fixed
order: a call repeated gives the same bits.  CPU tensors raise.

The moment form, for sets too large to hold (a standard FID: tens of thousands of samples, statistics of the real set kept).  A
``FrechetMoments`` keeps ``n``, the fp64 ``mean`` [D] and ``M`` = sum (x - mean)(x - mean)^T [D, D] of everything it has been fed,
batch by batch (each batch's centred scatter on the fp64 matrix pipe, joined by Chan's pairwise rule -- no raw second moments, so a
mean far from zero costs nothing), can be merged with another and saved.  ``factor()`` is F with F^T F = S = M / (n - 1), from the
same Jacobi iteration run on S itself; then tr sqrt(S1 S2) = ||F1 F2^T||_* and

    FD = |m1 - m2|^2 + tr S1 + tr S2 - 2 ||F1 F2^T||_*        (one D x D fp64 Gram and a third Jacobi solve)

D <= 4096, any N >= 2.  No D x D matrix leaves the device and nothing calls LAPACK.  Use it when N > D on both sides.  For N <= D the
covariance is singular, its zero eigenvalues come back as rounding noise of size u ||S|| and their square roots, of size sqrt(u), enter
the factor: the sample form above keeps its relative accuracy there and is the right tool (DESIGN.md section 4 has both bounds).

Not built: random-subset KID, distances across ranks (``merge`` makes that an all-gather), a two-solve variant through F1 S2 F1^T, a
one-launch solve for matrices that fit LDS, D > 4096."""
import ctypes as C

import torch

from . import _binding as B

MAX_SMALL, MAX_LARGE, MAX_SWEEPS, LDS_R = B.FC_FRECHET_MAX_SMALL, B.FC_FRECHET_MAX_LARGE, B.FC_JACOBI_MAX_SWEEPS, B.FC_JACOBI_LDS_R


def _rows(x, name):
    if not torch.is_tensor(x):
        raise TypeError(f"flocoder_amd.distances: {name} must be a tensor")
    if not x.is_cuda:
        raise RuntimeError(f"flocoder_amd.distances runs on MI355X (gfx950) only; there is no CPU path ({name} is a CPU tensor)")
    if x.dim() < 1:
        raise ValueError(f"flocoder_amd.distances: {name} must be [rows, ...]")
    return x.reshape(x.shape[0], -1).float().contiguous()


def _pair(a, b, names, min_rows, limits):
    """Both sets as fp32 rows on one device, shape-checked on the host: nothing is launched for a pair that a limit refuses."""
    a, b = _rows(a, names[0]), _rows(b, names[1])
    if a.device != b.device:
        raise ValueError(f"flocoder_amd.distances: {names[0]} and {names[1]} are on different devices")
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"flocoder_amd.distances: {names[0]} has {a.shape[1]} features, {names[1]} {b.shape[1]}")
    if a.shape[1] < 1 or a.shape[0] < min_rows or b.shape[0] < min_rows:
        raise ValueError(f"flocoder_amd.distances: each set needs at least {min_rows} row(s) and one feature, got {tuple(a.shape)} and {tuple(b.shape)}")
    small, large = sorted((a.shape[0], b.shape[0]))
    if small > limits[0] or large > limits[1]:
        raise ValueError(f"flocoder_amd.distances: min(N1, N2) <= {limits[0]} and max(N1, N2) <= {limits[1]}, got {a.shape[0]} and {b.shape[0]}")
    return a, b


def _workspace(what, n1, n2, dim, device):
    nbytes = B.lib().fc_frechet_workspace_bytes(what, n1, n2, dim)
    if nbytes < 0:
        B.check(int(nbytes))
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _moments(x):
    mean = torch.empty(x.shape[1], dtype=torch.float64, device=x.device)
    ssq = torch.empty(1, dtype=torch.float64, device=x.device)
    ws = _workspace(B.FC_WS_MOMENTS, x.shape[0], x.shape[0], x.shape[1], x.device)
    B.check(B.lib().fc_col_moments(B.ptr(x), x.shape[0], x.shape[1], B.ptr(mean), B.ptr(ssq), B.ptr(ws), B.current_stream(x.device)))
    return mean, ssq


def gram(a, b, center=False):
    """fp64 ``[N1, N2]``: ``sum_f a[i, f] b[j, f]``, or with ``center`` the same of the sets minus their own fp64 feature means."""
    a, b = _pair(a, b, ("a", "b"), 1, (B.FC_GRAM_MAX_ROWS, B.FC_GRAM_MAX_ROWS))
    out = torch.empty(a.shape[0], b.shape[0], dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        ma = _moments(a)[0] if center else None
        mb = (ma if b is a else _moments(b)[0]) if center else None
        B.check(B.lib().fc_gram_f64(B.ptr(a), a.shape[0], B.ptr(b), b.shape[0], a.shape[1], B.ptr(ma), B.ptr(mb), 1.0, B.ptr(out), None,
                                    None, B.current_stream(a.device)))
    return out


def singular_values(m):
    """``(svals [n] fp64 descending, info)`` of the fp64 device matrix ``m`` [n, r], by one-sided Jacobi on its rows; ``m`` is not
    modified.  ``info``: ``sweeps``, ``converged`` (False after a non-finite product or 30 sweeps: the values are then not singular
    values) and ``nuclear``, their sum as a 0-d device tensor."""
    if not torch.is_tensor(m) or m.dim() != 2 or m.dtype != torch.float64:
        raise ValueError("flocoder_amd.distances.singular_values: m must be a float64 tensor [n, r]")
    if not m.is_cuda:
        raise RuntimeError("flocoder_amd.distances runs on MI355X (gfx950) only; there is no CPU path (m is a CPU tensor)")
    n, r = m.shape
    if not 1 <= n <= MAX_SMALL or r < 1:
        raise ValueError(f"flocoder_amd.distances.singular_values: 1 <= n <= {MAX_SMALL} vectors of r >= 1 elements, got {tuple(m.shape)}")
    z = m.contiguous().clone()
    svals = torch.empty(n, dtype=torch.float64, device=m.device)
    nuclear = torch.empty(1, dtype=torch.float64, device=m.device)
    sweeps, converged = C.c_int(0), C.c_int(0)
    with torch.cuda.device(m.device):
        ws = _workspace(B.FC_WS_JACOBI, n, r, 1, m.device)
        B.check(B.lib().fc_jacobi_svals(B.ptr(z), n, r, B.ptr(svals), B.ptr(nuclear), B.ptr(ws), C.byref(sweeps), C.byref(converged),
                                        B.current_stream(m.device)))
    return svals, {"sweeps": sweeps.value, "converged": bool(converged.value), "nuclear": nuclear[0]}


def frechet_distance_sets(real, fake, return_info=False):
    """|mx - my|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2) between the sample sets ``real`` [N1, ...] and ``fake`` [N2, ...] (unbiased
    covariances), a Python float; ``(value, info)`` with ``return_info``.  Raises RuntimeError when the solve did not converge."""
    x, y = _pair(real, fake, ("real", "fake"), 2, (MAX_SMALL, MAX_LARGE))
    dev = x.device
    out = torch.empty(6, dtype=torch.float64, device=dev)
    svals = torch.empty(min(x.shape[0], y.shape[0]), dtype=torch.float64, device=dev) if return_info else None
    sweeps, converged, launches = C.c_int(0), C.c_int(0), C.c_int64(0)
    with torch.cuda.device(dev):
        ws = _workspace(B.FC_WS_FRECHET, x.shape[0], y.shape[0], x.shape[1], dev)
        B.check(B.lib().fc_frechet_sets(B.ptr(x), x.shape[0], B.ptr(y), y.shape[0], x.shape[1], B.ptr(ws), B.ptr(out), B.ptr(svals),
                                        C.byref(sweeps), C.byref(converged), C.byref(launches), B.current_stream(dev)))
    if not converged.value:
        raise RuntimeError(f"flocoder_amd.distances.frechet_distance_sets: the singular values did not converge in {sweeps.value} sweep(s) "
                           f"(a non-finite sample, or the cap of {MAX_SWEEPS} sweeps)")
    fd, dm2, t1, t2, nuc, _ = out.tolist()
    if not return_info:
        return fd
    return fd, {"sweeps": sweeps.value, "converged": True, "launches": launches.value, "mean_term": dm2, "trace_real": t1 if x.shape[0] <= y.shape[0] else t2,
                "trace_fake": t2 if x.shape[0] <= y.shape[0] else t1, "nuclear": nuc, "svals": svals}


def kernel_distance(real, fake):
    """The unbiased MMD^2 between ``real`` and ``fake`` with the cubic polynomial kernel k(x, y) = (x.y / D + 1)^3 (Binkowski et al.
    2018's KID estimator over all pairs), a Python float."""
    x, y = _pair(real, fake, ("real", "fake"), 2, (MAX_LARGE, MAX_LARGE))
    dev = x.device
    out = torch.empty(4, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        ws = _workspace(B.FC_WS_KID, x.shape[0], y.shape[0], x.shape[1], dev)
        B.check(B.lib().fc_kid_sets(B.ptr(x), x.shape[0], B.ptr(y), y.shape[0], x.shape[1], B.ptr(ws), B.ptr(out), B.current_stream(dev)))
    return out[0].item()


class FrechetMoments:
    """Running fp64 statistics of a sample set on the device: ``n``, ``mean`` [D] and ``M`` = sum (x - mean)(x - mean)^T [D, D].

    ``update(feats)`` takes a batch of rows (any shape, flattened per row, cast to fp32; the first call fixes ``dim`` and the device),
    ``merge(other)`` another state's samples.  ``covariance()`` is M / (n - 1), ``trace()`` its trace as a Python float, ``factor()``
    ``(F, eigenvalues, info)`` with F^T F = covariance, cached until the next ``update`` / ``merge`` / ``load_state_dict``."""

    def __init__(self):
        self.n, self.dim, self.mean, self.M = 0, None, None, None
        self._factor = None

    def _like(self, *shape):
        return torch.empty(*shape, dtype=torch.float64, device=self.mean.device)

    def update(self, feats):
        x = _rows(feats, "feats")
        nb, dim = x.shape
        if nb < 1 or not 1 <= dim <= MAX_SMALL:
            raise ValueError(f"flocoder_amd.distances.FrechetMoments: a batch is [rows >= 1, 1 <= features <= {MAX_SMALL}], got {tuple(x.shape)}")
        if self.dim is None:
            self.dim = dim
            self.mean = torch.empty(dim, dtype=torch.float64, device=x.device)
            self.M = torch.empty(dim, dim, dtype=torch.float64, device=x.device)
        elif dim != self.dim:
            raise ValueError(f"flocoder_amd.distances.FrechetMoments: the state has {self.dim} features, the batch {dim}")
        elif x.device != self.mean.device:
            raise ValueError("flocoder_amd.distances.FrechetMoments: the batch is on another device than the state")
        self._factor = None
        with torch.cuda.device(x.device):
            for r0 in range(0, nb, B.FC_GRAM_MAX_ROWS):
                part = x[r0:r0 + B.FC_GRAM_MAX_ROWS]
                ws = _workspace(B.FC_WS_MOMENTS_UPDATE, part.shape[0], 1, dim, x.device)
                B.check(B.lib().fc_frechet_moments_update(B.ptr(part), part.shape[0], dim, self.n, B.ptr(self.mean), B.ptr(self.M), B.ptr(ws),
                                                          B.current_stream(x.device)))
                self.n += part.shape[0]
        return self

    def merge(self, other):
        if not isinstance(other, FrechetMoments):
            raise TypeError("flocoder_amd.distances.FrechetMoments.merge: other must be a FrechetMoments")
        if other.n == 0:
            return self
        if self.dim is None:
            self.dim, self.mean, self.M = other.dim, torch.empty_like(other.mean), torch.empty_like(other.M)
        elif other.dim != self.dim:
            raise ValueError(f"flocoder_amd.distances.FrechetMoments.merge: {self.dim} features against {other.dim}")
        elif other.mean.device != self.mean.device:
            raise ValueError("flocoder_amd.distances.FrechetMoments.merge: the states are on different devices")
        self._factor = None
        dev = self.mean.device
        with torch.cuda.device(dev):
            ws = _workspace(B.FC_WS_MOMENTS_MERGE, 1, 1, self.dim, dev)
            B.check(B.lib().fc_frechet_moments_merge(self.dim, self.n, B.ptr(self.mean), B.ptr(self.M), other.n, B.ptr(other.mean), B.ptr(other.M),
                                                     B.ptr(ws), B.current_stream(dev)))
        self.n += other.n
        return self

    def _need(self, rows, what):
        if self.n < rows:
            raise ValueError(f"flocoder_amd.distances.FrechetMoments: {what} needs at least {rows} sample(s), the state has {self.n}")

    def covariance(self):
        self._need(2, "a covariance")
        return self.M * (1.0 / (self.n - 1))                             # the factor's own scaling: factor() reproduces exactly this matrix

    def trace(self):
        self._need(2, "a covariance")
        return float(self.M.diagonal().sum() / (self.n - 1)) if self._factor is None else float(self._factor[3])

    def factor(self):
        """``(F [D, D], eigenvalues [D] descending, info)``: F^T F = covariance(); ``info`` has ``sweeps``, ``converged``, ``launches`` and
        ``trace`` (a 1-element device tensor).  Raises RuntimeError when the solve did not converge."""
        self._need(2, "a factor")
        if self._factor is None:
            dev = self.mean.device
            f, ev, tr = self._like(self.dim, self.dim), self._like(self.dim), self._like(1)
            sweeps, converged, launches = C.c_int(0), C.c_int(0), C.c_int64(0)
            with torch.cuda.device(dev):
                ws = _workspace(B.FC_WS_MOMENTS_FACTOR, 1, 1, self.dim, dev)
                B.check(B.lib().fc_frechet_moments_factor(self.dim, self.n, B.ptr(self.M), B.ptr(f), B.ptr(ev), B.ptr(tr), B.ptr(ws),
                                                          C.byref(sweeps), C.byref(converged), C.byref(launches), B.current_stream(dev)))
            if not converged.value:
                raise RuntimeError(f"flocoder_amd.distances.FrechetMoments.factor: the eigenvalues did not converge in {sweeps.value} sweep(s) "
                                   f"(a non-finite sample, or the cap of {MAX_SWEEPS} sweeps)")
            self._factor = (f, ev, {"sweeps": sweeps.value, "converged": True, "launches": launches.value, "trace": tr}, tr)
        return self._factor[:3]

    def state_dict(self):
        if self.dim is None:
            raise ValueError("flocoder_amd.distances.FrechetMoments.state_dict: the state is empty")
        return {"n": torch.tensor(self.n, dtype=torch.int64), "mean": self.mean.clone(), "M": self.M.clone()}

    def load_state_dict(self, sd, device=None):
        n, mean, m = int(sd["n"]), sd["mean"], sd["M"]
        if mean.dim() != 1 or m.shape != (mean.shape[0], mean.shape[0]) or not 1 <= mean.shape[0] <= MAX_SMALL or n < 1:
            raise ValueError("flocoder_amd.distances.FrechetMoments.load_state_dict: n >= 1, mean [D], M [D, D], D <= 4096")
        device = device or (mean.device if mean.is_cuda else "cuda")
        self.n, self.dim = n, mean.shape[0]
        self.mean = mean.to(device=device, dtype=torch.float64).contiguous().clone()
        self.M = m.to(device=device, dtype=torch.float64).contiguous().clone()
        self._factor = None
        return self


def frechet_distance_moments(a, b, return_info=False):
    """The Frechet distance between the sets two ``FrechetMoments`` have seen (unbiased covariances), a Python float; ``(value, info)``
    with ``return_info``: ``sweeps`` (of a's factor, b's factor and the product), ``converged``, ``launches``, ``mean_term``,
    ``trace_real``, ``trace_fake``, ``nuclear``, ``svals``.  A factor already cached is not computed again."""
    for s, name in ((a, "a"), (b, "b")):
        if not isinstance(s, FrechetMoments):
            raise TypeError(f"flocoder_amd.distances.frechet_distance_moments: {name} must be a FrechetMoments")
        s._need(2, f"the distance ({name})")
    if a.dim != b.dim:
        raise ValueError(f"flocoder_amd.distances.frechet_distance_moments: a has {a.dim} features, b {b.dim}")
    if a.mean.device != b.mean.device:
        raise ValueError("flocoder_amd.distances.frechet_distance_moments: a and b are on different devices")
    cached = (a._factor is not None, b._factor is not None)
    (fa, _, ia), (fb, _, ib) = a.factor(), b.factor()
    dev, dim = a.mean.device, a.dim
    out = torch.empty(6, dtype=torch.float64, device=dev)
    svals = torch.empty(dim, dtype=torch.float64, device=dev) if return_info else None
    sweeps, converged, launches = C.c_int(0), C.c_int(0), C.c_int64(0)
    with torch.cuda.device(dev):
        ws = _workspace(B.FC_WS_MOMENTS_DISTANCE, 1, 1, dim, dev)
        B.check(B.lib().fc_frechet_moments_distance(dim, B.ptr(a.mean), B.ptr(fa), B.ptr(ia["trace"]), B.ptr(b.mean), B.ptr(fb), B.ptr(ib["trace"]),
                                                    B.ptr(ws), B.ptr(out), B.ptr(svals), C.byref(sweeps), C.byref(converged), C.byref(launches),
                                                    B.current_stream(dev)))
    if not converged.value:
        raise RuntimeError(f"flocoder_amd.distances.frechet_distance_moments: the singular values did not converge in {sweeps.value} sweep(s) "
                           f"(the cap of {MAX_SWEEPS} sweeps)")
    fd, dm2, t1, t2, nuc, _ = out.tolist()
    if not return_info:
        return fd
    spent = launches.value + (0 if cached[0] else ia["launches"]) + (0 if cached[1] else ib["launches"])
    return fd, {"sweeps": (ia["sweeps"], ib["sweeps"], sweeps.value), "converged": True, "launches": spent, "mean_term": dm2, "trace_real": t1,
                "trace_fake": t2, "nuclear": nuc, "svals": svals}
