"""The kernels that close a training step, each called through the C ABI and held to its fp64 reference with the derived bounds of
tests/step_pieces_ref.py (the inputs are that module's; tests/test_step_pieces_cpu.py shows torch's own fp32 arithmetic inside every
bound on them): the prologue (``fc_flow_prepare[_rows]``, ``fc_flow_interp``), the loss (``fc_mse_loss_grad[_scaled]``), the clip
(``fc_grad_clip_coef``), Adam + EMA (``fc_adam_ema_step[_guarded]``) in one call, at the buffer level, and over 200 steps.

Every output buffer is pre-filled with NaN and sits between guard zones: no NaN may survive inside, no bit may change outside.
Worst ratios of error to bound are printed per quantity (run with -s)."""
import pytest
import torch

import step_pieces_ref as R
from flocoder_amd import _binding as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
F32, F64 = torch.float32, torch.float64
NAN = float("nan")


class Buf:
    """n elements on the device between two guard zones of GUARD elements; ``init`` (a CPU tensor) or NaN / -1 inside, NaN / a
    sentinel in the guards."""

    def __init__(self, n, init=None, dtype=F32):
        fill = NAN if dtype == F32 else -0x5A5A5A5B
        self.n, self.dtype = n, dtype
        self.full = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        if init is not None:
            self.full[GUARD:GUARD + n] = init.reshape(-1).to(DEV)
        self.before = self.full.clone()

    @property
    def t(self):
        return self.full[GUARD:GUARD + self.n]

    @property
    def ptr(self):
        return self.full.data_ptr() + GUARD * self.full.element_size()

    def cpu(self):
        return self.t.cpu()

    def guards_intact(self):
        bits = torch.int32 if self.dtype == F32 else self.dtype
        a, b = self.full.view(bits), self.before.view(bits)
        return torch.equal(a[:GUARD], b[:GUARD]) and torch.equal(a[GUARD + self.n:], b[GUARD + self.n:])

    def unchanged(self):
        bits = torch.int32 if self.dtype == F32 else self.dtype
        return torch.equal(self.full.view(bits), self.before.view(bits))


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _dev(t):
    return None if t is None else t.contiguous().to(DEV)


def _stream():
    return B.current_stream(torch.device(DEV))


class Worst(dict):
    def add(self, key, got, ref, bound, case, failures):
        r = R.worst_ratio(got, ref, bound)
        self[key] = max(self.get(key, 0.0), r)
        if not r <= 1.0:
            failures.append(f"{case}: {key} at {r:.3f} of its bound")

    def show(self, title):
        for k, r in self.items():
            print(f"{title}: worst ratio of device error to bound, {k}: {r:.3f}")


# ---- prologue -------------------------------------------------------------------------------------------------------------------------
def _prepare_call(c, src, tgt, u, pairing, ids, flag_ptr, outs, warp_s=None, per=None):
    lib = B.lib()
    warp_s = c["warp_s"] if warp_s is None else warp_s
    per = c["per"] if per is None else per
    t, time, x, v = outs
    if c["rows_form"]:
        return lib.fc_flow_prepare_rows(B.ptr(src), B.ptr(tgt), B.ptr(pairing), B.ptr(u), R.T_EPS, warp_s, R.T_SCALE, B.ptr(ids), R.N_CLASSES,
                                        t.ptr, time.ptr, x.ptr, v.ptr, flag_ptr, c["batch"], c["first_row"], c["target_rows"], per, _stream())
    return lib.fc_flow_prepare(B.ptr(src), B.ptr(tgt), B.ptr(pairing), B.ptr(u), R.T_EPS, warp_s, R.T_SCALE, B.ptr(ids), R.N_CLASSES, t.ptr,
                               time.ptr, x.ptr, v.ptr, flag_ptr, c["batch"], per, _stream())


def test_prologue_against_fp64_with_pairing_class_id_and_row_range_variants():
    from flocoder_amd.sampling import warp_time
    lib = B.lib()
    worst, failures = Worst(), []
    t_scale32 = torch.tensor(R.T_SCALE, dtype=F32)
    for c in R.prologue_cases():
        name, batch, per = c["name"], c["batch"], c["per"]
        src, tgt, u, pairing, ids = (_dev(c[k]) for k in ("src", "tgt", "u", "pairing", "ids"))
        outs = [Buf(batch), Buf(batch), Buf(batch * per), Buf(batch * per)]
        flag = Buf(1, torch.zeros(1, dtype=torch.int32), dtype=torch.int32)
        assert _prepare_call(c, src, tgt, u, pairing, ids, flag.ptr if c["use_flag"] else None, outs) == B.FC_OK, name
        torch.cuda.synchronize()
        t, time, x, v = (o.cpu() for o in outs)
        for o, what in zip(outs, ("t", "time", "x", "v")):
            assert o.guards_intact(), (name, what, "guard zone written")
            assert not bool(torch.isnan(o.t).any()), (name, what, "an element was left unwritten")
        assert flag.guards_intact()
        ref = R.prepare(c["src"], c["tgt"], c["u"], R.T_EPS, c["warp_s"], R.T_SCALE, c["pairing"], c["ids"], R.N_CLASSES, c["first_row"],
                        c["target_rows"], t_for_x=t)
        assert int(flag.cpu()) == (ref["flag"] if c["use_flag"] else 0), (name, "flag bits", int(flag.cpu()), ref["flag"])
        if c["warp_s"] == 0.5:
            assert torch.equal(t, warp_time(c["u"] * (1 - R.T_EPS) + R.T_EPS)), (name, "t is not warp_time's")
        worst.add("t", t, ref["t"], R.t_bound(c["u"], R.T_EPS, c["warp_s"]), name, failures)
        assert torch.equal(time, t * t_scale32), (name, "time is not t * t_scale")
        worst.add("x", x.reshape(batch, per), ref["x"], ref["x_bound"], name, failures)
        g_rows = c["tgt"][ref["rows"]].contiguous()
        assert torch.equal(v.reshape(batch, per), g_rows - c["src"]), (name, "v* is not the rounded target - source")
        # the interpolation alone, on the gathered target and the t of above
        xi, vi = Buf(batch * per), Buf(batch * per)
        assert lib.fc_flow_interp(B.ptr(src), B.ptr(_dev(g_rows)), outs[0].ptr, xi.ptr, vi.ptr, batch, per, _stream()) == B.FC_OK, name
        torch.cuda.synchronize()
        assert xi.guards_intact() and vi.guards_intact(), (name, "interp: guard zone written")
        assert not bool(torch.isnan(xi.t).any() | torch.isnan(vi.t).any()), (name, "interp: an element was left unwritten")
        x_ref, _, x_bound = R.interp(c["src"], g_rows, t)
        worst.add("x (interp)", xi.cpu().reshape(batch, per), x_ref, x_bound, name, failures)
        assert torch.equal(vi.cpu().reshape(batch, per), g_rows - c["src"]), (name, "interp: v*")
    worst.show("prologue")
    assert not failures, failures


def test_prologue_refuses_what_would_read_out_of_bounds():
    """Refusals return before any launch: nothing is written."""
    lib = B.lib()
    c = dict(R.prologue_cases()[1])                                   # a rows-form case
    plain = dict(R.prologue_cases()[2])
    assert c["rows_form"] and not plain["rows_form"]
    for case in (c, plain):
        src, tgt, u = (_dev(case[k]) for k in ("src", "tgt", "u"))
        outs = [Buf(case["batch"]), Buf(case["batch"]), Buf(case["batch"] * case["per"]), Buf(case["batch"] * case["per"])]
        for s in (-0.1, 1.6):
            assert _prepare_call(case, src, tgt, u, None, None, None, outs, warp_s=s) == B.FC_E_ARG
        for per in (0, -1, 2 ** 31, 2 ** 32 + 1):
            assert _prepare_call(case, src, tgt, u, None, None, None, outs, per=per) == B.FC_E_ARG, per
            assert lib.fc_flow_interp(B.ptr(src), B.ptr(tgt), B.ptr(u), outs[2].ptr, outs[3].ptr, case["batch"], per, _stream()) == B.FC_E_ARG, per
        torch.cuda.synchronize()
        assert all(o.unchanged() for o in outs)
    g, out2, ws = _dev(torch.ones(8)), Buf(2), Buf(256)
    assert lib.fc_grad_clip_coef(B.ptr(g), -1, None, 0, 1.0, out2.ptr, ws.ptr, _stream()) == B.FC_E_ARG
    assert lib.fc_grad_clip_coef(B.ptr(g), 8, B.ptr(g), -1, 1.0, out2.ptr, ws.ptr, _stream()) == B.FC_E_ARG
    assert lib.fc_grad_clip_coef(B.ptr(g), -(2 ** 40), B.ptr(g), 8, 1.0, out2.ptr, ws.ptr, _stream()) == B.FC_E_ARG
    torch.cuda.synchronize()
    assert out2.unchanged() and ws.unchanged()


# ---- loss -----------------------------------------------------------------------------------------------------------------------------
def test_mse_loss_and_gradient_against_fp64():
    lib = B.lib()
    worst, failures = Worst(), []
    for name, v, tgt in R.loss_cases():
        n = v.numel()
        vd, td = _dev(v), _dev(tgt)
        dv, loss, ws = Buf(n), Buf(1), Buf(256)
        assert lib.fc_mse_loss_grad(B.ptr(vd), B.ptr(td), dv.ptr, loss.ptr, ws.ptr, n, _stream()) == B.FC_OK, name
        torch.cuda.synchronize()
        assert dv.guards_intact() and loss.guards_intact() and ws.guards_intact(), name
        assert bool(torch.isfinite(ws.t).all()), (name, "a workspace slot was left unwritten")
        assert not bool(torch.isnan(dv.t).any()), name
        ref_loss, ref_dv = R.mse(v, tgt)
        worst.add("loss", loss.cpu()[0], ref_loss, R.loss_rel_bound(n) * ref_loss, name, failures)
        worst.add("dv", dv.cpu(), ref_dv, R.dv_bound(ref_dv), name, failures)
        loss2, ws2 = Buf(1), Buf(256)                                 # dv = NULL: the loss alone, by the same arithmetic
        assert lib.fc_mse_loss_grad(B.ptr(vd), B.ptr(td), None, loss2.ptr, ws2.ptr, n, _stream()) == B.FC_OK, name
        torch.cuda.synchronize()
        assert _bits_equal(loss2.t, loss.t) and _bits_equal(ws2.t, ws.t) and loss2.guards_intact() and ws2.guards_intact(), name
    worst.show("loss")
    assert not failures, failures


def test_scaled_loss_over_unequal_micro_batches_is_the_whole_batch():
    lib = B.lib()
    worst, failures = Worst(), []
    v, tgt = R.micro_case()
    total = sum(R.MICRO_ROWS)
    whole_loss, whole_dv = R.mse(v, tgt)
    vd, td = _dev(v), _dev(tgt)
    dv, acc = Buf(v.numel()), Buf(1, torch.zeros(1))
    acc_only = Buf(1, torch.zeros(1))
    bound, lo = 0.0, 0
    for rows in R.MICRO_ROWS:
        n, off = rows * R.MICRO_PER, lo * R.MICRO_PER * 4
        for dv_ptr, a in ((dv.ptr + off, acc), (None, acc_only)):
            ws = Buf(256)
            assert lib.fc_mse_loss_grad_scaled(vd.data_ptr() + off, td.data_ptr() + off, dv_ptr, a.ptr, ws.ptr, n, rows / total, _stream()) == B.FC_OK
            torch.cuda.synchronize()
            assert bool(torch.isfinite(ws.t).all()) and ws.guards_intact()
        share = R.mse(v[lo:lo + rows], tgt[lo:lo + rows], rows / total)[0]
        # the share's own sum (one more rounding: the scale crosses the ABI as a float), then one U of the running value for the add
        bound += float(R.loss_rel_bound(n, extra=1) * share) + R.U * float(acc.cpu()[0])
        lo += rows
    assert dv.guards_intact() and acc.guards_intact() and not bool(torch.isnan(dv.t).any())
    assert _bits_equal(acc.t, acc_only.t), "the loss must not depend on whether dv is asked for"
    worst.add("micro-batch loss", acc.cpu()[0], whole_loss, bound, "3+1+2 rows", failures)
    worst.add("micro-batch dv", dv.cpu(), whole_dv, R.dv_bound(whole_dv), "3+1+2 rows", failures)
    worst.show("loss")
    assert not failures, failures


# ---- clip -----------------------------------------------------------------------------------------------------------------------------
def test_clip_norm_and_coefficient_against_fp64():
    lib = B.lib()
    worst, failures = Worst(), []
    for name, g, g2, max_norm in R.clip_cases():
        n, n2 = g.numel(), (0 if g2 is None else g2.numel())
        gd, g2d = _dev(g), _dev(g2)
        out2, ws = Buf(2), Buf(256)
        garbage = -7 if n % 2 else 2 ** 40 + 12345                    # numel2 without a second range: not looked at
        assert lib.fc_grad_clip_coef(B.ptr(gd), n, B.ptr(g2d), n2 if g2 is not None else garbage, max_norm, out2.ptr, ws.ptr,
                                     _stream()) == B.FC_OK, name
        torch.cuda.synchronize()
        assert out2.guards_intact() and ws.guards_intact() and bool(torch.isfinite(ws.t).all()), name
        norm, coef = R.clip(g, g2, max_norm)
        got_norm, got_coef = out2.cpu()
        worst.add("norm", got_norm, norm, R.norm_rel_bound(n, n2) * norm, name, failures)
        if float(coef) == 1.0:
            assert float(got_coef) == 1.0, (name, "the inactive clip's coefficient is exactly 1", float(got_coef))
        else:
            worst.add("coef", got_coef, coef, R.coef_rel_bound(n, n2) * coef, name, failures)
        if name == "zeros":
            assert float(got_norm) == 0.0
    worst.show("clip")
    assert not failures, failures


# ---- Adam + EMA -----------------------------------------------------------------------------------------------------------------------
HP = (R.B1, R.B2, R.EPS)


def _adam_call(bufs, n, coef_ptr, lr, step, apply_adam=1, skip_ptr=None, guarded=False, offset=0, decay=R.DECAY):
    """bufs: p, g, m, v, ema (Buf or None); ``offset`` elements into each."""
    ptrs = [None if b is None else b.ptr + 4 * offset for b in bufs]
    lib = B.lib()
    if guarded:
        return lib.fc_adam_ema_step_guarded(*ptrs, n, coef_ptr, lr, R.B1, R.B2, R.EPS, step, decay, apply_adam, skip_ptr, _stream())
    return lib.fc_adam_ema_step(*ptrs, n, coef_ptr, lr, R.B1, R.B2, R.EPS, step, decay, apply_adam, _stream())


def _adam_bufs(inputs):
    return [Buf(t.numel(), t) for t in inputs]


def test_adam_and_ema_one_call_against_fp64():
    worst, failures = Worst(), []
    for c in R.adam_cases():
        name, n = c["name"], c["n"]
        inputs = R.adam_inputs(n, c["state"], c["gscale"], c["seed"])
        p, g, m, v, ema = inputs
        bufs = _adam_bufs(inputs)
        coef = Buf(1, torch.tensor([c["coef"]], dtype=F32))
        assert _adam_call(bufs, n, coef.ptr, c["lr"], c["step"]) == B.FC_OK, name
        torch.cuda.synchronize()
        assert all(b.guards_intact() for b in bufs) and bufs[1].unchanged() and coef.unchanged(), name
        ref = R.adam_ema(p, g, m, v, ema, c["coef"], c["lr"], *HP, c["step"], R.DECAY)
        bounds = R.adam_bounds(g, m, ema, c["coef"], c["lr"], *HP, c["step"], ref)
        for key, i, r, bd in zip(("p", "exp_avg", "exp_avg_sq", "ema"), (0, 2, 3, 4), ref, bounds):
            worst.add(key, bufs[i].cpu(), r, bd, name, failures)
    worst.show("adam")
    assert not failures, failures


def test_adam_sub_range_at_a_four_byte_aligned_offset_leaves_the_rest_alone():
    """FlowTrainer walks the flat vectors in ranges [a, b) by pointer arithmetic: the start is 4-byte aligned and no more."""
    worst, failures = Worst(), []
    total, a, n = 4099 + 10, 3, 4099
    inputs = R.adam_inputs(total, "nonzero", 1e-4, 4900)
    bufs = _adam_bufs(inputs)
    coef = Buf(1, torch.tensor([0.37], dtype=F32))
    assert _adam_call(bufs, n, coef.ptr, 1e-3, 7, offset=a) == B.FC_OK
    torch.cuda.synchronize()
    sl = [t[a:a + n] for t in inputs]
    ref = R.adam_ema(*sl, 0.37, 1e-3, *HP, 7, R.DECAY)
    bounds = R.adam_bounds(sl[1], sl[2], sl[4], 0.37, 1e-3, *HP, 7, ref)
    for key, i, r, bd in zip(("p", "exp_avg", "exp_avg_sq", "ema"), (0, 2, 3, 4), ref, bounds):
        worst.add(key, bufs[i].cpu()[a:a + n], r, bd, "offset 3", failures)
        bits_now, bits_then = bufs[i].full.view(torch.int32), bufs[i].before.view(torch.int32)
        assert torch.equal(bits_now[:GUARD + a], bits_then[:GUARD + a]) and torch.equal(bits_now[GUARD + a + n:], bits_then[GUARD + a + n:]), key
    assert bufs[1].unchanged()
    worst.show("adam, sub-range")
    assert not failures, failures


def test_adam_guard_flag_null_arguments_and_empty_range():
    n = 4099
    inputs = R.adam_inputs(n, "nonzero", 1.0, 4901)
    p, g, m, v, ema = inputs
    coef = Buf(1, torch.tensor([0.37], dtype=F32))
    plain = _adam_bufs(inputs)
    assert _adam_call(plain, n, coef.ptr, 1e-4, 7) == B.FC_OK
    # skip flag set: nothing moves; clear: the unguarded call's bits
    for flag_value in (1, 2, 0):
        flag = Buf(1, torch.tensor([flag_value], dtype=torch.int32), dtype=torch.int32)
        bufs = _adam_bufs(inputs)
        assert _adam_call(bufs, n, coef.ptr, 1e-4, 7, skip_ptr=flag.ptr, guarded=True) == B.FC_OK
        torch.cuda.synchronize()
        assert flag.unchanged()
        if flag_value:
            assert all(b.unchanged() for b in bufs), "a flagged step must change nothing"
        else:
            assert all(_bits_equal(b.full, q.full) for b, q in zip(bufs, plain)), "flag 0 is the unguarded step"
    bufs = _adam_bufs(inputs)                                         # a NULL flag pointer: never skipped
    assert _adam_call(bufs, n, coef.ptr, 1e-4, 7, skip_ptr=None, guarded=True) == B.FC_OK
    torch.cuda.synchronize()
    assert all(_bits_equal(b.full, q.full) for b, q in zip(bufs, plain))
    # apply_adam = 0 with NULL gradient and moments: EMA only
    pb, eb = Buf(n, p), Buf(n, ema)
    assert _adam_call([pb, None, None, None, eb], n, None, 1e-4, 1, apply_adam=0) == B.FC_OK
    torch.cuda.synchronize()
    assert pb.unchanged() and eb.guards_intact()
    ref = R.adam_ema(p, g, m, v, ema, 1.0, 1e-4, *HP, 1, R.DECAY, apply_adam=False)
    r = R.worst_ratio(eb.cpu(), ref[3], R.adam_bounds(g, m, ema, 1.0, 1e-4, *HP, 1, ref, apply_adam=False)[3])
    print(f"adam: worst ratio of device error to bound, ema (no gradient): {r:.3f}")
    assert r <= 1.0
    # ema = NULL: Adam alone, the same bits
    bufs = _adam_bufs(inputs)
    assert _adam_call(bufs[:4] + [None], n, coef.ptr, 1e-4, 7) == B.FC_OK
    torch.cuda.synchronize()
    assert all(_bits_equal(b.full, q.full) for b, q in zip(bufs[:4], plain[:4])) and bufs[4].unchanged()
    # clip_coef_dev = NULL is a coefficient of 1.0f
    one = Buf(1, torch.ones(1))
    with_one, with_null = _adam_bufs(inputs), _adam_bufs(inputs)
    assert _adam_call(with_one, n, one.ptr, 1e-4, 7) == B.FC_OK and _adam_call(with_null, n, None, 1e-4, 7) == B.FC_OK
    torch.cuda.synchronize()
    assert all(_bits_equal(b.full, q.full) for b, q in zip(with_one, with_null))
    assert not _bits_equal(with_one[0].full, plain[0].full)           # and 0.37 was not 1
    # numel = 0: OK, nothing touched
    bufs = _adam_bufs(inputs)
    assert _adam_call(bufs, 0, coef.ptr, 1e-4, 7) == B.FC_OK and _adam_call(bufs, 0, coef.ptr, 1e-4, 7, guarded=True) == B.FC_OK
    torch.cuda.synchronize()
    assert all(b.unchanged() for b in bufs)


def test_two_hundred_steps_of_clip_adam_ema_drift_no_more_than_fp32_must():
    """clip -> Adam -> EMA for HORIZON_STEPS steps on the device alone, against the oracle's loop in fp64 and in fp32 (torch's own
    arithmetic) run here on the CPU.  A different rounding order gives errors of the oracle's size with independent sign: twice the
    fp32 oracle's own deviation from fp64 is the expected worst, the gate is 3 x.  Parameters and EMA are printed only (their
    rounding swamps any drift; the one-call bounds gate them)."""
    lib = B.lib()
    p0, grads = R.horizon_inputs()
    n = R.HORIZON_N
    ref, norms = R.horizon_oracle(p0, grads, F64)
    o32, _ = R.horizon_oracle(p0, grads, F32)
    active = sum(nm > R.HORIZON_MAX_NORM for nm in norms)
    assert 20 < active < R.HORIZON_STEPS - 20, active
    gd = _dev(grads)
    bufs = [Buf(n, p0), None, Buf(n, torch.zeros(n)), Buf(n, torch.zeros(n)), Buf(n, p0)]
    out2, ws = Buf(2), Buf(256)
    for s in range(R.HORIZON_STEPS):
        g_ptr = gd.data_ptr() + 4 * n * s
        assert lib.fc_grad_clip_coef(g_ptr, n, None, 0, R.HORIZON_MAX_NORM, out2.ptr, ws.ptr, _stream()) == B.FC_OK
        assert lib.fc_adam_ema_step(bufs[0].ptr, g_ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, n, out2.ptr + 4, R.HORIZON_LR, R.B1, R.B2, R.EPS,
                                    s + 1, R.DECAY, 1, _stream()) == B.FC_OK
    torch.cuda.synchronize()
    assert all(b.guards_intact() for b in bufs if b is not None)
    got = (bufs[0].cpu().to(F64), bufs[2].cpu().to(F64), bufs[3].cpu().to(F64), bufs[4].cpu().to(F64))
    dv, dm, dp, de = R.horizon_figures(got, ref)
    ov, om, op, oe = R.horizon_figures(o32, ref)
    print(f"horizon: {R.HORIZON_STEPS} steps, clip active on {active}")
    print(f"horizon: exp_avg_sq worst relative deviation from fp64: device {dv:.3e}, fp32 oracle {ov:.3e}, ratio {dv / ov:.2f}")
    print(f"horizon: exp_avg worst absolute deviation from fp64: device {dm:.3e}, fp32 oracle {om:.3e}, ratio {dm / om:.2f}")
    print(f"horizon: parameters worst absolute deviation from fp64: device {dp:.3e}, fp32 oracle {op:.3e} (not gated)")
    print(f"horizon: ema worst absolute deviation from fp64: device {de:.3e}, fp32 oracle {oe:.3e} (not gated)")
    assert dv <= 3 * ov, (dv, ov)
    assert dm <= 3 * om, (dm, om)
