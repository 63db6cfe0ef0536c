"""flocoder_amd.sampling.log_likelihood / invert_latents on the CPU: the generic-model (torch) path, which documents the formulas the
library's loop implements, against closed forms and against the fp64 restatement over the oracle U-Net (tests/likelihood_ref.py).

Bounds: the closed-form cases derive theirs from RK4's truncation error (stated at each test); the U-Net case in fp32 is held to the gate
of the GPU test (tests/test_gpu_likelihood.py): TRAJ_TOL on z, and on a the backward's per-sample d(x) tolerance G_TOL carried through
Cauchy-Schwarz, ``likelihood_ref.a_bound``."""
import math

import pytest
import torch

import likelihood_ref as lr
from conftest import load_golden
from flocoder_amd import sampling as S
from flocoder_amd.metrics import bits_per_dim
from oracle.synth import synth_input, synth_state_dict

G_TOL = 2e-6            # tests/unet_grad_taps.py: per-sample gate of every activation gradient, d(x) included
TRAJ_TOL = 2e-4         # tests/test_gpu_unet.py: trajectories of up to 64 forwards


def _rel(a, b):
    a, b = a.double().flatten(1), b.double().flatten(1)
    return (a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-300)


def test_constant_diagonal_field_gives_minus_trace_exactly_and_rk4_accurate_noise():
    """v(x, t) = s (.) x with s per channel: the Jacobian is diag(s), a Rademacher probe makes every d_j = sum(s) exactly, so
    a = sum(s) * sum(dt) = -sum(s) whatever the grid.  z_i = x_i prod_k R(h_k), h_k = s_i dt_k, R the degree-4 Taylor polynomial of exp;
    telescoping prod R_k - prod e^{h_k} with |R(h)|, e^h <= e^|h| and |e^h - R(h)| <= |h|^5/120 e^|h| (Lagrange remainder) gives
    |z_i - x_i e^{-s_i}| <= |x_i| e^{|s_i|} sum_k (|s_i| |dt_k|)^5 / 120 (sum |dt_k| = 1: the warped grid is monotone)."""
    s = torch.tensor([0.7, -0.4, 1.0, 0.25], dtype=torch.float64)
    sv = s.view(1, 4, 1, 1)
    model = lambda x, time, cond=None: sv * x
    x = synth_input("ll.diag", (3, 4, 6, 6), 1).double()
    tr = float(s.sum()) * 36
    for n in (2, 5, 12, 50):
        logp, z, nfe = S.log_likelihood(model, x, n_steps=n, generator=torch.Generator().manual_seed(n))
        assert nfe == 4 * (n - 1) and logp.dtype == torch.float64 and z.dtype == torch.float64
        a = logp + 0.5 * z.flatten(1).pow(2).sum(1) + 0.5 * 144 * math.log(2 * math.pi)
        assert float((a + tr).abs().max()) <= 1e-12 * abs(tr), (n, a, tr)
        dts = S.rk4_time_grid(n, dtype=torch.float64).diff().abs()
        bound = x.abs() * sv.abs().exp() * ((sv.abs() * dts.view(-1, 1, 1, 1, 1)) ** 5 / 120).sum(0) + 1e-14 * x.abs()
        err = (z - x * (-sv).exp()).abs()
        assert bool((err <= bound).all()), (n, float((err / bound).max()))
        if n <= 5:                      # the bound is not vacuous: the truncation error is there and within an order of it
            assert float((err / bound).max()) > 1e-3


def test_gaussian_to_gaussian_flow_returns_the_target_log_density_at_fourth_order():
    """v(x, t) = x (sigma - 1) / (1 + (sigma - 1) t) carries N(0, I) at t = 0 to N(0, sigma^2 I) at t = 1; logp must be the N(0, sigma^2 I)
    log-density of the input, which pins every sign.  The error is discretisation only (diagonal Jacobian, Rademacher probe), so it falls
    with the order of the method: a factor >= 8 from 17 to 33 grid points, and at 33 below 1e-5 |exact| (only a wrong formula misses that)."""
    sigma, shape = 2.5, (4, 4, 4, 4)
    D = 64
    x = sigma * synth_input("ll.gauss", shape, 2).double()
    exact = -0.5 * x.flatten(1).pow(2).sum(1) / sigma ** 2 - 0.5 * D * math.log(2 * math.pi * sigma ** 2)

    def model(xx, time, cond=None):
        t = (time / 999).view(-1, 1, 1, 1)
        return xx * (sigma - 1) / (1 + (sigma - 1) * t)

    err = {}
    for n in (5, 9, 17, 33):
        logp, z, _ = S.log_likelihood(model, x, n_steps=n, generator=torch.Generator().manual_seed(7))
        err[n] = float((logp - exact).abs().max())
    print("gaussian flow, max |logp - exact| by n_steps:", err)
    assert err[17] / err[33] >= 8, err
    assert err[33] <= 1e-5 * float(exact.abs().min()), (err, exact)
    assert err[5] > err[9] > err[17]
    bpd = bits_per_dim(exact, D)
    assert torch.allclose(bpd, -exact / (D * math.log(2.0))) and bool((bpd > 0).all())


def _unet_case():
    sd = synth_state_dict(load_golden("g3_unet_d16c10")["shapes"], 2)
    x = synth_input("ll.x.d16c10", (3, 4, 16, 16), 2)
    eps = torch.where(synth_input("ll.eps.d16c10", (3, 4, 16, 16), 2) >= 0, 1.0, -1.0)
    cls = torch.tensor([1, 7, 4])
    return sd, x, eps, {"class_cond": cls}


@pytest.mark.timeout(900)
def test_generic_path_on_the_oracle_unet_equals_the_restatement():
    sd, x, eps, cond = _unet_case()
    sd64 = {k: v.double() for k, v in sd.items()}
    ref = lr.log_likelihood_ref(sd64, x.double(), 9, cond, eps.double())
    logp, z, nfe = S.log_likelihood(lr.oracle_model(sd64), x.double(), n_steps=9, cond=cond, probe=eps.double())
    assert nfe == 32 and len(ref.stages) == 32
    a = logp + 0.5 * z.flatten(1).pow(2).sum(1) + 0.5 * 1024 * math.log(2 * math.pi)
    assert float(((logp - ref.logp).abs() / ref.logp.abs()).max()) <= 1e-12
    assert float(((a - ref.a).abs() / ref.a.abs()).max()) <= 1e-9      # a is recovered from logp here: |a| << |logp|
    assert float(_rel(z, ref.z).max()) <= 1e-12
    logp_b, _, a_b, _ = S._log_likelihood_torch(lr.oracle_model(sd64), x.double(), lr.reversed_grid(9, torch.float64), cond, eps.double())
    assert float(((a_b - ref.a).abs() / ref.a.abs()).max()) <= 1e-12 and torch.equal(logp_b, logp)

    # fp32: the gate of the GPU test
    logp32, z32, a32, _ = S._log_likelihood_torch(lr.oracle_model(sd), x, lr.reversed_grid(9, torch.float32), cond, eps)
    assert z32.dtype == torch.float32 and a32.dtype == torch.float64
    bound = lr.a_bound(ref, eps, G_TOL)
    ratio = (a32 - ref.a).abs() / bound
    zr = _rel(z32, ref.z)
    print(f"fp32 oracle against fp64: |a - a64| / bound {ratio.tolist()}, z rel-L2 {zr.tolist()}, a64 {ref.a.tolist()}, bound {bound.tolist()}")
    assert bool((ratio <= 1).all()), ratio
    assert float(zr.max()) < TRAJ_TOL
    lb = bound + 0.5 * (z32.double().flatten(1).pow(2).sum(1) - ref.z.flatten(1).pow(2).sum(1)).abs()
    assert bool(((logp32 - ref.logp).abs() <= lb).all())
    pub, _, _ = S.log_likelihood(lr.oracle_model(sd), x, n_steps=9, cond=cond, probe=eps)
    assert torch.equal(pub, logp32)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("n", [9, 5])
def test_inversion_round_trip_is_the_restatements_round_trip(n):
    """invert_latents, then the oracle's forward RK4 on the same grid, comes back to the input up to the discretisation error of the two
    solves -- the error the restatement's own round trip has; the two round trips are compared with each other, not with zero."""
    sd, x, _, cond = _unet_case()
    sd64 = {k: v.double() for k, v in sd.items()}
    z, nfe = S.invert_latents(lr.oracle_model(sd64), x.double(), n_steps=n, cond=cond)
    assert nfe == 4 * (n - 1)
    z_ref = lr.invert_ref(sd64, x.double(), n, cond)
    assert float(_rel(z, z_ref).max()) <= 1e-12
    back, back_ref = lr.forward_ref(sd64, z, n, cond), lr.forward_ref(sd64, z_ref, n, cond)
    rt, rt_ref = float(_rel(back, x).max()), float(_rel(back_ref, x).max())
    print(f"n={n}: round trip error {rt:.3e}, restatement's {rt_ref:.3e}")
    assert abs(rt - rt_ref) <= 1e-9 * rt_ref and 0 < rt_ref < 2e-2
    z32, _ = S.invert_latents(lr.oracle_model(sd), x, n_steps=n, cond=cond["class_cond"])      # bare class ids, as the legacy samplers take them
    assert z32.dtype == torch.float32 and float(_rel(z32, z_ref).max()) < TRAJ_TOL


def test_argument_errors():
    model = lambda x, time, cond=None: -x
    x = torch.zeros(2, 4, 4, 4)
    with pytest.raises(ValueError, match="guidance"):
        S.log_likelihood(model, x, n_steps=4, cfg_strength=3.0)
    with pytest.raises(ValueError, match="shape"):
        S.log_likelihood(model, x, n_steps=4, probe=torch.ones(2, 4, 4, 5))
    with pytest.raises(ValueError, match="n_steps"):
        S.log_likelihood(model, x, n_steps=1)
    with pytest.raises(ValueError, match="n_steps"):
        S.invert_latents(model, x, n_steps=1)
    with pytest.raises(ValueError, match="probe"):
        S.log_likelihood(model, x, n_steps=4, probe="sobol")
    S.log_likelihood(model, x, n_steps=3, cfg_strength=0.0)
    S.log_likelihood(model, x, n_steps=3, cfg_strength=None, probe="gaussian")
    from flocoder_amd.unet import Unet
    m = Unet(dim=8, channels=4, n_classes=0).eval()
    with pytest.raises(RuntimeError):
        S.log_likelihood(m, torch.zeros(1, 4, 8, 8), n_steps=3)
    with pytest.raises(RuntimeError):
        S.invert_latents(m, torch.zeros(1, 4, 8, 8), n_steps=3)


def test_model_state_is_left_as_found_and_probes_are_reproducible():
    torch.manual_seed(0)
    net = torch.nn.Conv2d(4, 4, 3, padding=1)

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.net = net

        def forward(self, x, time, cond=None):
            return self.net(x) * 0.1

    m = M().train()
    x = synth_input("ll.state", (2, 4, 6, 6), 3)
    g = lambda: torch.Generator().manual_seed(11)
    l1, z1, _ = S.log_likelihood(m, x, n_steps=4, generator=g())
    l2, z2, _ = S.log_likelihood(m, x, n_steps=4, generator=g())
    assert torch.equal(l1, l2) and torch.equal(z1, z2)
    assert m.training and all(p.requires_grad and p.grad is None for p in m.parameters())
    for p in m.parameters():
        p.requires_grad_(False)
    l3, _, _ = S.log_likelihood(m.eval(), x, n_steps=4, generator=g())
    assert torch.equal(l1, l3) and not m.training and not any(p.requires_grad for p in m.parameters())
    lg, _, _ = S.log_likelihood(m, x, n_steps=4, probe="gaussian", generator=g())
    assert not torch.equal(lg, l1)
