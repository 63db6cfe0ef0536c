"""Gradient accumulation, validation loss and ``set_lr`` of ``FlowTrainer`` on the GPU (``fc_unet_backward_accumulate``,
``fc_mse_loss_grad_scaled``, ``fc_flow_prepare_rows``).

Models come from the goldens: ``g3_unet_d16c10`` at 4x16x16 (class conditioning) and ``g3_unet_d8mask`` at 4x8x8 (mask branches).  Six rows,
so that micro-batches of four leave a ragged chunk of two: a chunk that fills the plan's batch takes the table-driven weight-gradient
launches, the ragged one the per-layer launches, and both have to add.

Gates.  Accumulated gradients against ``oracle.train_oracle.loss_and_grads`` in fp64 on the WHOLE batch: per-parameter rel-L2 < 2e-5 and
|loss - ref| < 2e-6 ref, the figures tests/test_gpu_train.py holds a one-batch backward to against the same oracle, for every parameter
without exception (measured worst 8.7e-6).  Accumulated against the whole-batch GPU backward: < 4e-5, both being within 2e-5 of one
reference (measured worst 7.7e-7).  Everything that is "the same computation" is compared bit for bit.
Measured values are printed with -s."""
import functools
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from conftest import load_golden, rel_l2
from oracle import train_oracle as to
from oracle.synth import synth_input, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 6
PAIRING = [5, 3, 0, 4, 1, 2]                 # every chunk of (4, 2) and of (2, 2, 2) reaches into another chunk's target rows
CASES = ["cls", "nocond", "pairing", "mask", "ones"]
SPLITS = [(4, 2), (2, 2, 2)]


def _shapes(case):
    return load_golden("g3_unet_d8mask" if case in ("mask", "ones") else "g3_unet_d16c10")["shapes"]


def _sd(case):
    return synth_state_dict(_shapes(case), 3)


def _model(case):
    from flocoder_amd.unet import Unet
    kw = dict(dim=8, n_classes=0, mask_cond=True) if case in ("mask", "ones") else dict(dim=16, n_classes=10)
    m = Unet(channels=4, dim_mults=(1, 2, 4, 8), **kw)
    m.load_state_dict(_sd(case), strict=True)
    return m.to(DEV).train()


def _trainer(case, **kw):
    from flocoder_amd.train import FlowTrainer
    return FlowTrainer(_model(case), **kw)


@functools.lru_cache(maxsize=None)
def _data(case):
    """(source, target, u, class ids | None, mask | None, pairing | None) on the host."""
    hw = 8 if case in ("mask", "ones") else 16
    src, tgt = synth_input(f"acc.src.{hw}", (N, 4, hw, hw), 3), synth_input(f"acc.tgt.{hw}", (N, 4, hw, hw), 3)
    u = torch.sigmoid(synth_input("acc.u", (N,), 3, scale=1.5))
    cls = torch.tensor([1, 7, 4, 0, 9, 7]) if case in ("cls", "pairing") else None
    mask = None
    if case == "mask":
        mask = torch.sigmoid(synth_input("acc.mask", (N, 4, hw, hw), 3, scale=2.0))
    if case == "ones":
        mask = torch.ones(N, 4, hw, hw)
    pairing = torch.tensor(PAIRING) if case == "pairing" else None
    return src, tgt, u, cls, mask, pairing


def _cond(cls, mask, rows=slice(None)):
    if cls is None and mask is None:
        return None
    return {"class_cond": None if cls is None else cls[rows], "mask_cond": None if mask is None else mask[rows]}


def _oracle(case, rows=slice(None)):
    """fp64 loss and gradients of the oracle on ``rows`` of the case's batch (the whole batch by default)."""
    src, tgt, u, cls, mask, pairing = _data(case)
    if pairing is not None:
        tgt = tgt[pairing]
    sd64 = {k: v.double() for k, v in _sd(case).items()}
    t = to.train_time(u)                                   # fp32, as the prologue computes it
    cond = _cond(cls, None if mask is None else mask.double(), rows)
    loss, grads, _ = to.loss_and_grads(sd64, src[rows].double(), tgt[rows].double(), t[rows].double(), cond)
    return loss, grads


@functools.lru_cache(maxsize=None)
def _ref(case):
    return _oracle(case)


def _accumulate(tr, case, split):
    src, tgt, u, cls, mask, pairing = _data(case)
    a = 0
    for n in split:
        rows = slice(a, a + n)
        tr.accumulate(src[rows], tgt, _cond(cls, mask, rows), u=u[rows], pairing=None if pairing is None else pairing[rows], of_total=N)
        a += n


def _check_grads(model, flat, grads_ref, tol, scale=1.0, only=None):
    views = model.grad_views(flat)
    total = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads_ref.values() if g is not None)))
    worst = ("", 0.0)
    for k, gr in grads_ref.items():
        if only is not None and not k.startswith(only):
            continue
        got = views[k].cpu()
        if gr is None:
            assert float(got.abs().max()) == 0.0, k
            continue
        e = rel_l2(got, gr * scale)
        worst = max(worst, (k, e), key=lambda kv: kv[1])
        assert e < tol, (k, e, float(gr.norm()), total)
    return worst


def _state(tr):
    return {k: getattr(tr, k).clone() for k in ("params", "exp_avg", "exp_avg_sq", "ema")}


def _same_state(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


# ---- gradients ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", SPLITS, ids=lambda s: "+".join(map(str, s)))
@pytest.mark.parametrize("case", CASES)
def test_accumulated_gradients_match_the_oracle_on_the_whole_batch(case, split):
    loss_ref, grads_ref = _ref(case)
    tr = _trainer(case)
    _accumulate(tr, case, split)
    worst = _check_grads(tr.model, tr.grads, grads_ref, 2e-5)
    loss = float(tr.apply())
    print(case, split, "worst parameter gradient:", worst, "loss", loss, "ref", float(loss_ref))
    assert abs(loss - float(loss_ref)) < 2e-6 * float(loss_ref)
    assert tr.step_main == 1


@pytest.mark.parametrize("case", CASES)
def test_accumulated_gradients_agree_with_the_whole_batch_backward(case):
    src, tgt, u, cls, mask, pairing = (None if v is None else v.to(DEV) for v in _data(case))
    whole = _trainer(case)
    t, time, x, v_t = whole.prepare(src, tgt, u, cls, pairing)
    whole.loss_and_grads(x, t, cls, v_t, mask, time=time)
    ref = {k: v.cpu() for k, v in whole.model.grad_views(whole.grads).items()}
    for split in SPLITS:
        tr = _trainer(case)
        _accumulate(tr, case, split)
        worst = ("", 0.0)
        for k, got in tr.model.grad_views(tr.grads).items():
            if float(ref[k].abs().max()) == 0.0:
                assert float(got.abs().max()) == 0.0, k
                continue
            e = rel_l2(got.cpu(), ref[k])
            worst = max(worst, (k, e), key=lambda kv: kv[1])
            assert e < 4e-5, (case, split, k, e)
        print(case, split, "worst against the whole-batch backward:", worst)
        tr.discard()


def test_mixed_presence_class_range_holds_the_conditioned_chunk_alone():
    src, tgt, u, cls, _, _ = _data("cls")
    _, grads4 = _oracle("cls", slice(0, 4))
    tr = _trainer("cls")
    tr.accumulate(src[:4], tgt, {"class_cond": cls[:4]}, u=u[:4], of_total=N)
    tr.accumulate(src[4:], tgt, None, u=u[4:], of_total=N)
    worst = _check_grads(tr.model, tr.grads, grads4, 2e-5, scale=4.0 / N, only="class_cond_mlp.")
    print("class range against the oracle on the conditioned rows x 4/6:", worst)
    tr.apply()
    assert tr.steps["class"] == 1 and tr.step_main == 1


def test_step_without_ids_leaves_the_class_range_untouched():
    src, tgt, u, _, _, _ = _data("nocond")
    tr = _trainer("nocond")
    lo, hi = tr._groups["class"]
    assert hi > lo
    before = {k: v.clone() for k, v in _state(tr).items() if k != "ema"}
    tr.step(src, tgt, None, u=u, micro_batch=4)
    after = _state(tr)
    assert all(torch.equal(before[k][lo:hi], after[k][lo:hi]) for k in before)
    assert tr.steps["class"] == 0 and tr.step_main == 1
    assert not torch.equal(before["params"][hi:], after["params"][hi:]) and float(tr.exp_avg[hi:].abs().max()) > 0     # the rest did step


@pytest.mark.parametrize("case", ["nocond", "mask_dropped"])
def test_accumulating_backward_touches_only_what_has_a_gradient(case):
    """The C entry on a sentinel vector: padding and the ranges without a gradient in this call (class_cond_mlp.* without ids, the mask
    branches without a mask) keep their bits; everything else is sentinel + g with g the overwriting backward's bits."""
    data_case = "nocond" if case == "nocond" else "mask"
    src, tgt, u, _, _, _ = (None if v is None else v.to(DEV) for v in _data(data_case))
    tr = _trainer(data_case)
    m = tr.model
    t, time, x, v_t = tr.prepare(src[:4].contiguous(), tgt[:4].contiguous(), u[:4].contiguous())
    _, v = tr.loss_and_grads(x, t, None, v_t, None, time=time)            # leaves the forward in the arena and g in tr.grads
    g = tr.grads.clone()
    dv = (2.0 / v.numel()) * (v - v_t)
    n = g.numel()
    sentinel = (1000.0 + (torch.arange(n, device=DEV) % 97).float()) * torch.where(torch.arange(n, device=DEV) % 2 == 0, 1.0, -1.0)
    acc = sentinel.clone()
    m.backward_native(x, time, None, dv, acc, accumulate=True)
    covered = torch.zeros(n, dtype=torch.bool, device=DEV)
    quiet = ("class_cond_mlp.",) if case == "nocond" else ("mask_fusion_conv.", "down_mask_fusions.", "up_mask_fusions.")
    n_quiet = 0
    for name, shape, off in m._table:
        numel = 1
        for s_ in shape:
            numel *= s_
        if name.startswith(quiet):
            n_quiet += numel
        else:
            covered[off:off + numel] = True
    assert n_quiet > 0 and int((~covered).sum()) >= n_quiet               # a gradient-less range (and whatever padding the table has) to look at
    assert torch.equal(acc[~covered], sentinel[~covered])
    g2 = torch.empty_like(g)
    m.backward_native(x, time, None, dv, g2)                              # the overwriting entry for the same d(out)
    assert float(g2[~covered].abs().max()) == 0.0
    assert torch.equal(acc[covered], (sentinel + g2)[covered])
    assert rel_l2(g2, g) < 1e-6                                           # ... which is the step's gradient (d(out) rebuilt in torch)


def test_accumulated_step_is_deterministic():
    src, tgt, u, cls, _, pairing = _data("pairing")
    runs = []
    for _ in range(2):
        tr = _trainer("pairing")
        loss = tr.step(src, tgt, {"class_cond": cls}, u=u, pairing=pairing, micro_batch=4)
        runs.append((_state(tr), tr.grads.clone(), loss.clone()))
    assert _same_state(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


def test_step_without_micro_batch_is_the_existing_pieces():
    src, tgt, u, cls, _, pairing = (None if v is None else v.to(DEV) for v in _data("pairing"))
    a, b = _trainer("pairing"), _trainer("pairing")
    for _ in range(2):
        loss_a = a.step(src, tgt, {"class_cond": cls}, u=u, pairing=pairing)
        t, time, x, v_t = b.prepare(src, tgt, u, cls, pairing)
        loss_b, _ = b.loss_and_grads(x, t, cls, v_t, None, time=time)
        loss_b = loss_b.clone()
        b.optimizer_step(has_class_grads=True)
        assert torch.equal(loss_a, loss_b)
    assert _same_state(_state(a), _state(b)) and a.steps == b.steps and a.step_main == b.step_main == 2


def test_three_accumulated_steps_match_reference_golden():
    """The three steps of fixture g10 (reference Unet + torch.optim.Adam + EMA 0.999, step 2 unconditioned) with micro_batch = half its
    batch, under the gates ``test_three_training_steps_match_reference_golden`` applies to the one-batch step."""
    g = load_golden("g10_train_step")
    from flocoder_amd.train import FlowTrainer
    from flocoder_amd.unet import Unet
    m = Unet(dim=16, channels=4, dim_mults=(1, 2, 4, 8), n_classes=10)
    m.load_state_dict(synth_state_dict(g["shapes"], 10))
    m = m.to(DEV).train()
    tr = FlowTrainer(m, lr=1e-4, ema_decay=0.999)
    cls = torch.from_numpy(g["cls"]).to(DEV)
    worst = 0.0
    for step in (1, 2, 3):
        src, tgt = synth_input(f"g10.src{step}", (8, 4, 16, 16), 10), synth_input(f"g10.tgt{step}", (8, 4, 16, 16), 10)
        u = torch.sigmoid(synth_input(f"g10.u{step}", (8,), 10, scale=1.5))
        cond = {"class_cond": cls, "mask_cond": None} if step != 2 else None
        loss = tr.step(src, tgt, cond, u=u, micro_batch=4)
        print("step", step, "loss", float(loss), "golden", float(g[f"s{step}_loss"]), "norm", float(tr.grad_norm), "golden", float(g[f"s{step}_norm"]))
        assert abs(float(loss) - float(g[f"s{step}_loss"])) < 5e-6 * float(g[f"s{step}_loss"]), step
        assert abs(float(tr.grad_norm) - float(g[f"s{step}_norm"])) < 1e-4 * float(g[f"s{step}_norm"]), step
        sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        ema = {k: v.cpu() for k, v in tr.ema_state_dict().items()}
        for i, k in enumerate(list(g["names"])):
            assert abs(float(sd[k].double().sum()) - g[f"s{step}_psum"][i]) <= 3e-6 * g[f"s{step}_pabs"][i] + 1e-9, (step, k)
            assert abs(float(ema[k].double().sum()) - g[f"s{step}_esum"][i]) <= 3e-6 * g[f"s{step}_eabs"][i] + 1e-9, (step, k)
        for k in g["small"]:
            e = rel_l2(sd[k], g[f"s{step}_param_{k}"])
            worst = max(worst, e)
            assert e < 2e-6, (step, k, e)
    print("worst parameter rel-L2 against the golden:", worst)
    assert tr.step_main == 3 and tr.step_class == 2
    assert m.reserved_rows() == 4


def test_only_the_micro_batch_is_ever_reserved():
    src, tgt, u, cls, _, pairing = _data("pairing")
    tr = _trainer("pairing")
    m = tr.model
    assert m.reserved_rows() == 0
    tr.step(src, tgt, {"class_cond": cls}, u=u, pairing=pairing, micro_batch=2)
    assert m.reserved_rows() == 2
    serial = m.arena_serial()
    loss = tr.step(src, tgt, {"class_cond": cls}, u=u, pairing=pairing, micro_batch=2)
    assert m.reserved_rows() == 2 and m.arena_serial() == serial + 3     # three forwards of two rows, no re-plan
    assert torch.isfinite(loss) and tr.step_main == 2


# ---- validation loss, learning rate ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["pairing", "mask"])
def test_eval_loss_equals_the_oracle_and_changes_nothing(case):
    src, tgt, u, cls, mask, pairing = _data(case)
    loss_ref, _ = _ref(case)
    cond = _cond(cls, mask)
    tr, twin = _trainer(case), _trainer(case)
    for t_ in (tr, twin):
        t_.step(src, tgt, cond, u=u, pairing=pairing)           # Adam / EMA state and gradients worth comparing
    loss_ref2, _, _ = to.loss_and_grads({k: v.detach().cpu().double() for k, v in tr.model.state_dict().items()},
                                     src.double(), (tgt if pairing is None else tgt[pairing]).double(), to.train_time(u).double(),
                                     _cond(cls, None if mask is None else mask.double()))
    before, grads, counters, training = _state(tr), tr.grads.clone(), (tr.step_main, dict(tr.steps)), tr.model.training
    for mb in (None, 4):
        loss = tr.eval_loss(src, tgt, cond, u=u, pairing=pairing, micro_batch=mb)
        print(case, "micro_batch", mb, "eval loss", float(loss), "ref", float(loss_ref2))
        assert loss.dim() == 0 and loss.device.type == "cuda"
        assert abs(float(loss) - float(loss_ref2)) < 2e-6 * float(loss_ref2)
    assert float(loss_ref2) != float(loss_ref)                   # (the step moved the weights: the reference is the trained model's)
    assert _same_state(before, _state(tr)) and torch.equal(grads, tr.grads)
    assert counters == (tr.step_main, dict(tr.steps)) and tr.model.training == training
    la, lb = tr.step(src, tgt, cond, u=u, pairing=pairing), twin.step(src, tgt, cond, u=u, pairing=pairing)
    assert torch.equal(la, lb) and _same_state(_state(tr), _state(twin))


def test_eval_loss_on_a_fresh_trainer_matches_the_oracle():
    src, tgt, u, cls, _, pairing = _data("pairing")
    loss_ref, _ = _ref("pairing")
    tr = _trainer("pairing")
    for mb in (4, None):
        loss = tr.eval_loss(src, tgt, {"class_cond": cls}, u=u, pairing=pairing, micro_batch=mb)
        assert abs(float(loss) - float(loss_ref)) < 2e-6 * float(loss_ref), (mb, float(loss), float(loss_ref))
    assert tr.step_main == 0 and float(tr.grads.abs().max()) == 0.0


def test_set_lr_moves_both_groups_of_an_inpainting_step():
    from flocoder_amd.inpainting import MaskEncoder
    from flocoder_amd.train import FlowTrainer
    from flocoder_amd.unet import Unet

    def make(lr):
        torch.manual_seed(31)
        model, me = Unet(dim=8, channels=4, dim_mults=(1, 2, 4, 8), n_classes=0, mask_cond=True).to(DEV).train(), MaskEncoder().to(DEV).train()
        tr = FlowTrainer(model, lr=lr)
        tr.attach_mask_encoder(me)
        return tr
    lr = 1e-3
    a, b = make(lr), make(lr / 2)
    a.set_lr(lr / 2)
    assert a.lr == b.lr and a.me_lr == b.me_lr == (lr / 2) * 0.1
    gen = torch.Generator().manual_seed(32)
    tgt, s0, noise = (torch.randn(3, 4, 8, 8, generator=gen).to(DEV) for _ in range(3))
    pix = (torch.rand(3, 1, 128, 128, generator=gen) > 0.5).float().to(DEV)
    u = torch.rand(3, generator=gen).to(DEV)
    start = a.params.clone(), a.me_params.clone()
    la, lb = a.inpaint_step(s0, tgt, pix, noise=noise, u=u), b.inpaint_step(s0, tgt, pix, noise=noise, u=u)
    assert torch.equal(la, lb) and torch.equal(a.params, b.params) and torch.equal(a.me_params, b.me_params)
    assert not torch.equal(a.params, start[0]) and not torch.equal(a.me_params, start[1])


# ---- bad inputs ------------------------------------------------------------------------------------------------------------------
def test_pairing_index_out_of_range_in_a_later_chunk_blocks_the_step():
    src, tgt, u, cls, _, pairing = _data("pairing")
    tr = _trainer("pairing")
    before = _state(tr)
    bad = pairing.clone()
    bad[5] = N                                                   # in the second chunk; N - 1 would be fine, the chunk's own size is 2
    with pytest.raises(IndexError):
        tr.step(src, tgt, {"class_cond": cls}, u=u, pairing=bad, micro_batch=4)
        tr.check_class_ids()
    torch.cuda.synchronize()
    assert _same_state(before, _state(tr))
    tr.step(src, tgt, {"class_cond": cls}, u=u, pairing=pairing, micro_batch=4)      # 5 in the second chunk is in range: N, not the chunk, bounds it
    tr.check_class_ids()
    assert not torch.equal(before["params"], tr.params)


def test_bad_arguments():
    src, tgt, u, cls, _, _ = _data("cls")
    tr = _trainer("cls")
    for mb in (0, -3):
        with pytest.raises(ValueError):
            tr.step(src, tgt, {"class_cond": cls}, u=u, micro_batch=mb)
    with pytest.raises(RuntimeError):
        tr.apply()
    tr.accumulate(src[:4], tgt, {"class_cond": cls[:4]}, u=u[:4], of_total=N)
    with pytest.raises(ValueError):
        tr.apply()                                               # four rows of a step declared with six
    with pytest.raises(RuntimeError):
        tr.apply()                                               # ... and that step is gone
    tr.accumulate(src[:4], tgt, {"class_cond": cls[:4]}, u=u[:4], of_total=N)
    tr.discard()
    with pytest.raises(RuntimeError):
        tr.apply()
    assert tr.step_main == 0 and float(tr.exp_avg.abs().max()) == 0.0


# ---- data parallel ---------------------------------------------------------------------------------------------------------------
HALF, MICRO = 8, 4


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dp_data():
    g = torch.Generator().manual_seed(2025)
    n = 2 * HALF
    src, tgt = torch.randn(2, n, 4, 16, 16, generator=g), torch.randn(2, n, 4, 16, 16, generator=g)       # [step][sample]
    u = torch.rand(2, n, generator=g)
    ids = torch.randint(10, (2, n), generator=g)
    pair = torch.stack([torch.stack([torch.randperm(HALF, generator=g) for _ in range(2)]) for _ in range(2)])   # [step][rank][HALF]
    return src, tgt, u, ids, pair


def _dp_worker(rank, world, port, q, outdir):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    from flocoder_amd import dist as fdist
    fdist.init(backend="gloo")
    calls = [0]
    real = dist.all_reduce

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    dist.all_reduce = counted
    tr = _trainer("cls", lr=1e-3, ema_decay=0.9)
    assert tr.distributed
    src, tgt, u, ids, pair = _dp_data()
    lo, hi = rank * HALF, (rank + 1) * HALF
    losses, before_last = [], []
    for step in range(2):
        s, t_, uu, cc, pp = (v.to(DEV) for v in (src[step, lo:hi], tgt[step, lo:hi], u[step, lo:hi], ids[step, lo:hi], pair[step, rank]))
        drop = step == 1 and rank == 1                         # this rank dropped its conditioning, the other did not
        n0 = calls[0]
        tr.accumulate(s[:MICRO], t_, None if drop else {"class_cond": cc[:MICRO]}, u=uu[:MICRO], pairing=pp[:MICRO], of_total=HALF)
        before_last.append(calls[0] - n0)
        tr.accumulate(s[MICRO:], t_, None if drop else {"class_cond": cc[MICRO:]}, u=uu[MICRO:], pairing=pp[MICRO:], of_total=HALF)
        losses.append(float(tr.apply()))
        assert calls[0] > n0
    torch.cuda.synchronize()
    torch.save((tr.params.cpu(), tr.ema.cpu(), tr.exp_avg.cpu(), tr.exp_avg_sq.cpu()), os.path.join(outdir, f"rank{rank}.pt"))
    q.put((rank, losses, dict(tr.steps), tr.step_main, before_last))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_of_two_micro_batches_equal_one_process(tmp_path):
    """tests/test_gpu_dist_train.py's comparison (gloo, two ranks on one GPU, rank 1 without conditioning in the second step) with every
    rank's half taken as two micro-batches, under that file's tolerances; no all-reduce runs before a step's last micro-batch."""
    tr = _trainer("cls", lr=1e-3, ema_decay=0.9, distributed=False)
    src, tgt, u, ids, pair = _dp_data()
    ref_losses = []
    for step in range(2):
        pairing = torch.cat([pair[step, 0], HALF + pair[step, 1]]).to(DEV)
        cls = ids[step].clone()
        if step == 1:
            cls[HALF:] = -1                                     # rank 1's rows carry no class in that step
        t, time, x, v_t = tr.prepare(src[step].to(DEV), tgt[step].to(DEV), u[step].to(DEV), None, pairing)
        loss, _ = tr.loss_and_grads(x, t, cls.to(DEV), v_t, None, time=time)
        ref_losses.append(float(loss))
        tr.optimizer_step(has_class_grads=True)
    torch.cuda.synchronize()
    ref = (tr.params.cpu(), tr.ema.cpu(), tr.exp_avg.cpu(), tr.exp_avg_sq.cpu())
    del tr

    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=500) for _ in procs), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    r0, r1 = res
    t0, t1 = (torch.load(os.path.join(str(tmp_path), f"rank{r}.pt")) for r in range(2))
    for a, b in zip(t0, t1):
        assert torch.equal(a, b), "replicas must stay bit-identical"
    assert r0[2] == r1[2] == {"class": 2, "fusion": 0, "inject": 0} and r0[3] == r1[3] == 2
    assert r0[4] == r1[4] == [0, 0], "no collective before a step's last micro-batch"
    errs = [rel_l2(a, b) for a, b in zip(t0, ref)]
    mean_loss = [(a + b) / 2 for a, b in zip(r0[1], r1[1])]
    print("DP x micro-batches vs single process: params %.2e ema %.2e exp_avg %.2e exp_avg_sq %.2e; losses %s vs %s" % (*errs, mean_loss, ref_losses))
    assert errs[0] < 2e-6 and errs[1] < 2e-6, errs
    assert errs[2] < 1e-5 and errs[3] < 1e-5, errs
    for a, b in zip(mean_loss, ref_losses):
        assert abs(a - b) <= 2e-6 * abs(b)
