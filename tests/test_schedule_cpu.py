"""``general.CosineAnnealingWarmRestartsDecay`` (train_flow.py:319,456: T_0=50, T_mult=2, decay=0.6, stepped once per epoch) against
``torch.optim.lr_scheduler.CosineAnnealingWarmRestarts`` -- the schedule it decays the base of -- and against the closed form of the
decayed cycles.  Host arithmetic in Python floats: 1e-12 relative is the bound of the comparison with torch's own doubles."""
import math

import pytest
import torch

from flocoder_amd.general import CosineAnnealingWarmRestartsDecay


class _Holder:
    def __init__(self, lr):
        self.lr = lr
        self.seen = []

    def set_lr(self, lr):
        self.lr = lr
        self.seen.append(lr)


@pytest.mark.parametrize("T_0,T_mult", [(50, 2), (30, 1)])
def test_without_decay_it_is_torchs_warm_restarts(T_0, T_mult):
    base = 3e-4
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=base)
    ref = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=T_0, T_mult=T_mult, eta_min=1e-6)
    h = _Holder(base)
    sch = CosineAnnealingWarmRestartsDecay(h, T_0=T_0, T_mult=T_mult, eta_min=1e-6, decay=1.0)
    for epoch in range(400):
        want = opt.param_groups[0]["lr"]
        assert abs(h.lr - want) <= 1e-12 * want, (epoch, h.lr, want)
        assert sch.get_last_lr() == [h.lr]
        opt.step()
        ref.step()
        sch.step()


def test_base_decays_at_every_restart_and_the_cycle_follows_the_cosine():
    base, T_0, T_mult, decay = 1e-4, 50, 2, 0.6
    h = _Holder(base)
    sch = CosineAnnealingWarmRestartsDecay(h, T_0=T_0, T_mult=T_mult, decay=decay)
    lrs = []
    for _ in range(T_0 + 2 * T_0 + 4 * T_0):
        lrs.append(h.lr)
        sch.step()
    starts = [0, T_0, T_0 + 2 * T_0]                      # first epoch of cycles 0, 1, 2
    for k, e in enumerate(starts):
        assert lrs[e] == pytest.approx(base * decay ** k, rel=1e-12), (k, lrs[e])
    for k, (e, T_i) in enumerate(zip(starts, (T_0, 2 * T_0, 4 * T_0))):
        b = base * decay ** k
        for j in range(T_i):
            assert lrs[e + j] == pytest.approx(b * (1 + math.cos(math.pi * j / T_i)) / 2, rel=1e-12, abs=1e-30), (k, j)
    assert lrs[T_0 - 1] < 1e-3 * base                       # the end of a cycle is the bottom of the cosine, not the decayed base


def test_two_setters_keep_their_ratio():
    a, b = _Holder(None), _Holder(None)
    sch = CosineAnnealingWarmRestartsDecay([(a.set_lr, 1e-4), (b.set_lr, 1e-5)], T_0=5, T_mult=2, decay=0.6)
    for _ in range(40):
        assert a.lr == pytest.approx(10 * b.lr, rel=1e-12, abs=1e-30)
        sch.step()
    assert len(a.seen) == len(b.seen) == 41


def test_state_round_trip_and_bad_arguments():
    h = _Holder(1e-3)
    sch = CosineAnnealingWarmRestartsDecay(h, T_0=4, T_mult=2, decay=0.5)
    for _ in range(7):
        sch.step()
    h2 = _Holder(1e-3)
    twin = CosineAnnealingWarmRestartsDecay(h2, T_0=4, T_mult=2, decay=0.5)
    twin.load_state_dict(sch.state_dict())
    for _ in range(9):
        assert h.lr == h2.lr
        sch.step()
        twin.step()
    with pytest.raises(ValueError):
        CosineAnnealingWarmRestartsDecay(h, T_0=0)
    with pytest.raises(ValueError):
        CosineAnnealingWarmRestartsDecay(h, T_0=5, T_mult=0)
