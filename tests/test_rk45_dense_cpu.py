"""Dense output of the adaptive RK45 sampler (``t_eval`` of rk45_sampler / generate_latents_rk45 / Unet.integrate_rk45) on the host: a
plain torch field goes through scipy's own ``solve_ivp(..., t_eval=...)``, so its frames are scipy's bit for bit while the final latents
and nfe stay those of the call without ``t_eval``; the argument checks raise scipy's messages before anything else, without a GPU; and
the stored oracle trajectories (tests/golden/rk45_dense_scipy_oracle.npz) are the solves of the two older RK45 fixtures."""
import numpy as np
import pytest
import torch
from torch import nn

from conftest import load_golden, rel_l2
from flocoder_amd import sampling as S

TE = [1e-3, 0.05, 0.25, 0.5, 0.75, 0.9, 1.0]
TRAJ_TOL, NFEV_SLACK = 2e-4, 12           # the gates of tests/test_gpu_rk45.py


class SinField(nn.Module):
    """v = -k x + sin(t), t = time / 999 as the samplers hand it over; k = 1, or 1 + 4 * class id with class ids (per-sample stiffness)."""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.ones(()))

    def forward(self, x, time, cond=None):
        t = (time / 999.0).view(-1, 1, 1, 1)
        k = 1.0
        if cond and cond.get("class_cond") is not None:
            k = 1.0 + 4.0 * cond["class_cond"].float().view(-1, 1, 1, 1)
        return self.w * (-k * x) + torch.sin(t)


def _scipy_frames(model, z0, cond, te, eps=1e-3, rtol=1e-5, atol=1e-5):
    """solve_ivp(..., t_eval=te) as the legacy sampler would call it: (y cast to fp32 as [F, *shape], nfev)."""
    from scipy import integrate
    shape = tuple(z0.shape)

    def f(t, y):
        x = torch.from_numpy(y.reshape(shape)).type(torch.float32)
        return model(x, torch.ones(shape[0]) * t * 999, cond).detach().numpy().reshape(-1)

    sol = integrate.solve_ivp(f, (eps, 1), z0.numpy().reshape(-1), rtol=rtol, atol=atol, method="RK45", t_eval=te)
    assert sol.success and sol.y.shape[1] == len(te)
    return torch.tensor(sol.y.T.copy()).reshape((len(te),) + shape).type(torch.float32), int(sol.nfev)


def test_frames_are_scipys_and_latents_are_unchanged():
    model = SinField()
    z0 = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(3))
    lat, nfe, frames = S.rk45_sampler(model, tuple(z0.shape), source=z0, t_eval=TE)
    ref, ref_nfe = _scipy_frames(model, z0, None, TE)
    assert frames.dtype == torch.float32 and frames.shape == (len(TE),) + tuple(z0.shape)
    assert torch.equal(frames, ref) and nfe == ref_nfe
    plain, plain_nfe = S.rk45_sampler(model, tuple(z0.shape), source=z0)
    assert torch.equal(lat, plain) and nfe == plain_nfe
    assert torch.equal(frames[0], z0)                                   # t_eval[0] == t0: y0
    assert rel_l2(frames[-1], lat) < 1e-6                               # the interpolant at t1, not y_new: equal to rounding
    # generate_latents_rk45 passes it through
    lat2, nfe2, frames2 = S.generate_latents_rk45(model, tuple(z0.shape), cfg_strength=0.0, source=z0, t_eval=np.asarray(TE))
    assert torch.equal(lat2, lat) and nfe2 == nfe and torch.equal(frames2, frames)


def test_per_sample_frames_are_one_scipy_solve_per_sample():
    model = SinField()
    z0 = torch.randn(3, 4, 4, 4, generator=torch.Generator().manual_seed(21))
    ids = torch.tensor([0, 3, 9])
    lat, nfe, frames = S.rk45_sampler(model, tuple(z0.shape), cond=ids, source=z0, per_sample=True, t_eval=torch.tensor(TE, dtype=torch.float64))
    nfevs = []
    for b in range(3):
        ref, n = _scipy_frames(model, z0[b:b + 1], {"class_cond": ids[b:b + 1]}, TE)
        assert torch.equal(frames[:, b:b + 1], ref), b
        nfevs.append(n)
    assert len(set(nfevs)) == 3 and nfe == max(nfevs)                   # the samples really take different steps
    plain, plain_nfe = S.rk45_sampler(model, tuple(z0.shape), cond=ids, source=z0, per_sample=True)
    assert torch.equal(lat, plain) and nfe == plain_nfe


BAD = [([[0.1, 0.2]], "`t_eval` must be 1-dimensional."),
       (0.5, "`t_eval` must be 1-dimensional."),
       ([0.1, 1.5], "Values in `t_eval` are not within `t_span`."),
       ([1e-4, 0.5], "Values in `t_eval` are not within `t_span`."),
       ([0.5, 0.25], "Values in `t_eval` are not properly sorted."),
       ([0.25, 0.25], "Values in `t_eval` are not properly sorted.")]


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("te,msg", BAD)
def test_argument_errors_on_a_plain_model(te, msg, per_sample):
    calls = []

    class Counting(SinField):
        def forward(self, x, time, cond=None):
            calls.append(1)
            return super().forward(x, time, cond)

    z0 = torch.zeros(1, 4, 2, 2)
    with pytest.raises(ValueError) as e:
        S.rk45_sampler(Counting(), tuple(z0.shape), source=z0, per_sample=per_sample, t_eval=te)
    assert str(e.value) == msg and not calls                            # scipy's message, raised before the model is called


@pytest.mark.parametrize("te,msg", BAD)
def test_argument_errors_on_a_cpu_unet_come_before_no_cpu_path(te, msg):
    from flocoder_amd.unet import Unet
    torch.manual_seed(0)
    m = Unet(dim=8, dim_mults=(1, 2), channels=4, n_classes=0).eval()
    z0 = torch.zeros(1, 4, 8, 8)
    with pytest.raises(ValueError) as e:
        S.generate_latents_rk45(m, tuple(z0.shape), source=z0, t_eval=te)
    assert str(e.value) == msg
    with pytest.raises(ValueError) as e:
        m.integrate_rk45(z0.clone(), 1e-3, 1.0, rtol=1e-5, atol=1e-5, t_eval=te)
    assert str(e.value) == msg


def test_good_times_on_a_cpu_unet_reach_no_cpu_path():
    from flocoder_amd.unet import Unet
    torch.manual_seed(0)
    m = Unet(dim=8, dim_mults=(1, 2), channels=4, n_classes=0).eval()
    z0 = torch.zeros(1, 4, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.generate_latents_rk45(m, tuple(z0.shape), source=z0, t_eval=TE)
    # backwards: decreasing times are the sorted ones, increasing ones are not
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.integrate_rk45(z0.clone(), 1.0, 1e-3, rtol=1e-5, atol=1e-5, t_eval=TE[::-1])
    with pytest.raises(ValueError, match="not properly sorted"):
        m.integrate_rk45(z0.clone(), 1.0, 1e-3, rtol=1e-5, atol=1e-5, t_eval=TE)


@pytest.mark.parametrize("per_sample", [False, True])
def test_empty_t_eval_gives_no_frames_and_the_same_latents(per_sample):
    model = SinField()
    z0 = torch.randn(2, 4, 4, 4, generator=torch.Generator().manual_seed(5))
    lat, nfe, frames = S.rk45_sampler(model, tuple(z0.shape), source=z0, per_sample=per_sample, t_eval=[])
    assert frames.shape == (0, 2, 4, 4, 4) and frames.dtype == torch.float32
    plain, plain_nfe = S.rk45_sampler(model, tuple(z0.shape), source=z0, per_sample=per_sample)
    assert torch.equal(lat, plain) and nfe == plain_nfe


@pytest.mark.parametrize("mode,name", [("coupled", "d16_cfg3"), ("coupled", "d8mask"), ("coupled", "d32"),
                                       ("per_sample", "d16_mixed"), ("per_sample", "d8mask")])
def test_fixture_is_the_solve_of_the_older_fixtures(mode, name):
    """The trajectories were recorded from the very solves of rk45_scipy_oracle.npz / rk45_per_sample_scipy_oracle.npz: nfev within
    NFEV_SLACK and final latents within TRAJ_TOL of those files (equal bits when generated on one machine; the oracle's forward is not
    promised bit-stable across hosts).  t_eval[0] == t0, so frame 0 is the source exactly."""
    d = load_golden("rk45_dense_scipy_oracle")
    old = load_golden("rk45_scipy_oracle" if mode == "coupled" else "rk45_per_sample_scipy_oracle")
    key = f"{mode}.{name}"
    assert d[f"{key}.t_eval"].tolist() == TE
    assert np.array_equal(d[f"{key}.source"], old[f"{name}.source"])
    frames, src = d[f"{key}.frames"], d[f"{key}.source"]
    assert frames.dtype == np.float32 and frames.shape == (len(TE),) + src.shape and np.isfinite(frames).all()
    assert np.array_equal(frames[0], src)
    new_counts, old_counts = d[f"{key}.counts"].reshape(-1, 3), old[f"{name}.counts"].reshape(-1, 3)
    assert new_counts.shape == old_counts.shape
    assert np.abs(new_counts[:, 0] - old_counts[:, 0]).max() <= NFEV_SLACK, (new_counts.tolist(), old_counts.tolist())
    lat, old_lat = d[f"{key}.latents"], old[f"{name}.latents"]
    rows = range(lat.shape[0]) if mode == "per_sample" else [slice(None)]
    for r in rows:
        assert rel_l2(lat[r], old_lat[r]) < TRAJ_TOL, (r, rel_l2(lat[r], old_lat[r]))
        assert rel_l2(frames[-1][r], lat[r]) < 1e-6                     # the interpolant at t1 against the solver's y(t1)
