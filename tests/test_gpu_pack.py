"""The weight packer (csrc/pack.hip pack_table_kernel, through fc_debug_pack) against the NumPy restatement of its ten layouts
(tests/pack_ref.py, itself checked by tests/test_pack_cpu.py): byte equality, no tolerance -- eight layouts are permutations, the two
folded-upsample layouts add in a stated fp32 order and the split is an integer rule.  Shapes are the smallest at which each can go wrong:
sizes that are no multiple of the 256 threads or of the 4096 elements of a table block, more than one block, padding on either side, a
slice in the middle of a wider buffer.  Every destination sits between sentinels that must survive."""
import ctypes as C

import numpy as np
import pytest
import torch

import pack_ref as pr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7777.0
GUARD = 16


def _src(seed, kind, dims):
    return np.random.default_rng(seed).standard_normal(pr.src_floats(kind, dims)).astype(np.float32)


def _split_src(seed, kind, dims):
    """N(0, 1) with the split's edge cases planted: +0, -0, a value exact in bf16 (remainder 0), the ties 1 + 2^-8 and 1 + 3 * 2^-8."""
    x = _src(seed, kind, dims)
    x[3:8] = [0.0, -0.0, 1.5, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8]
    return x


def _job(seed, kind, *dims, slot=None, src=_src):
    """(kind, dims, source, destination before the job: `slot` floats (default: what the library reports) of sentinel)."""
    return kind, dims, src(seed, kind, dims), np.full(slot or pr.dst_floats(kind, dims), SENTINEL, np.float32)


JOBS = {
    "conv_two_blocks": _job(1, pr.PACK_CONV, 24, 20, 9),                  # 4320 elements: a full block and a partial one, no multiple of 256
    "conv_below_a_wave": _job(2, pr.PACK_CONV, 4, 4, 1),
    "s2d": _job(3, pr.PACK_S2D, 8, 4),
    "transpose_slice": _job(4, pr.PACK_TRANSPOSE, 12, 8, 20, 5),
    "copy_slot": _job(5, pr.PACK_COPY, 5, slot=8),
    "pad_both": _job(6, pr.PACK_CONV_PAD, 3, 3, 9, 4, 4),
    "pad_in": _job(7, pr.PACK_CONV_PAD, 6, 3, 9, 8, 4),
    "dgrad_slice": _job(8, pr.PACK_DGRAD, 8, 12, 3, 4, 8),
    "dgrad_1x1": _job(9, pr.PACK_DGRAD, 8, 12, 1, 0, 12),
    "k8_three_blocks": _job(10, pr.PACK_CONV_K8, 32, 32, 9),
    "k8_1x1": _job(11, pr.PACK_CONV_K8, 32, 32, 1),
    "b3": _job(12, pr.PACK_CONV_B3, 8, 20, 9, 32, src=_split_src),
    "up4": _job(13, pr.PACK_UP4, 8, 20),
    "up4_b3": _job(14, pr.PACK_UP4_B3, 8, 20, 32),
}
# neighbours of different kinds, the multi-block jobs in the middle of the (job, block) map
INTERLEAVED = ["copy_slot", "k8_three_blocks", "b3", "conv_below_a_wave", "up4_b3", "transpose_slice", "conv_two_blocks", "dgrad_slice",
               "pad_both", "up4", "s2d", "k8_1x1", "dgrad_1x1", "pad_in"]


def _run(jobs, launch=True):
    """fc_debug_pack on [(kind, dims, src, dst0)] -> (return code, [destination with its guards as int32 bits], reported sizes)."""
    from flocoder_amd import _binding as B
    n = len(jobs)
    kinds = (C.c_int * n)(*[j[0] for j in jobs])
    dims = (C.c_int * (5 * n))(*[d for j in jobs for d in (list(j[1]) + [0] * 5)[:5]])
    srcs = [torch.from_numpy(j[2]).to(DEV) for j in jobs]
    dsts = [torch.from_numpy(np.concatenate([np.full(GUARD, SENTINEL, np.float32), j[3], np.full(GUARD, SENTINEL, np.float32)])).to(DEV) for j in jobs]
    sp = (C.c_void_p * n)(*[t.data_ptr() for t in srcs])
    dp = (C.c_void_p * n)(*[t.data_ptr() + 4 * GUARD for t in dsts])
    sizes = (C.c_int64 * n)(*([-1] * n))
    torch.cuda.synchronize()
    rc = B.lib().fc_debug_pack(n, kinds, dims, sp if launch else None, dp if launch else None, sizes, B.current_stream(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, [t.cpu().numpy().view(np.int32) for t in dsts], list(sizes)


def _want(job):
    kind, dims, src, dst0 = job
    body = pr.pack(kind, dims, src, dst=dst0)
    body = np.concatenate([body, dst0[body.size:]])                        # a slot wider than the job keeps its tail
    g = np.full(GUARD, SENTINEL, np.float32)
    return np.concatenate([g, body, g]).view(np.int32)


def _check(names):
    jobs = [JOBS[k] for k in names]
    rc, got, sizes = _run(jobs)
    assert rc == 0
    assert sizes == [pr.dst_floats(j[0], j[1]) for j in jobs]
    for name, job, g in zip(names, jobs, got):
        want = _want(job)
        assert g.shape == want.shape and np.array_equal(g, want), f"{name}: {int((g != want).sum())} of {want.size} words differ"


def test_the_split_cases_keep_every_remainder_zero_or_normal():
    """What the comparison below rests on: how the device subtraction treats denormals is not pinned, so the inputs avoid them."""
    tiny = np.finfo(np.float32).tiny
    for name in ("b3", "up4_b3"):
        kind, dims, src, _ = JOBS[name]
        parts = pr.pack(kind, dims, src).view(np.uint16)
        vals = np.abs(pr.bf16_to_f32(parts))
        assert np.all((vals == 0) | (vals >= tiny)), name
    x = JOBS["b3"][2].reshape(8, 20, 9)
    hi, lo = pr.split_bf16(x.reshape(-1)[3:8])
    assert hi.tolist() == [0x0000, 0x8000, 0x3fc0, 0x3f80, 0x3f82] and lo[:3].tolist() == [0, 0, 0] and lo[3] != 0 and lo[4] != 0


@pytest.mark.parametrize("name", list(JOBS))
def test_each_layout_alone_equals_the_restatement(name):
    _check([name])


def test_all_layouts_interleaved_in_one_table():
    assert sorted(INTERLEAVED) == sorted(JOBS)
    _check(INTERLEAVED)


def test_sizes_are_reported_without_a_launch():
    jobs = [JOBS[k] for k in JOBS]
    rc, got, sizes = _run(jobs, launch=False)
    assert rc == 0 and sizes == [pr.dst_floats(j[0], j[1]) for j in jobs]
    assert all(np.all(g.view(np.float32) == SENTINEL) for g in got)


@pytest.mark.parametrize("bad", [pr.N_KINDS, -1, 7777])
def test_a_kind_outside_the_enum_is_refused_and_nothing_is_launched(bad):
    from flocoder_amd import _binding as B
    good = JOBS["conv_below_a_wave"]
    rc, got, _ = _run([good, (bad, (4, 4, 1), good[2], good[3]), good])
    assert rc == B.FC_E_ARG and b"layout" in B.lib().fc_last_error()
    assert all(np.all(g.view(np.float32) == SENTINEL) for g in got)         # the valid neighbours did not run either
