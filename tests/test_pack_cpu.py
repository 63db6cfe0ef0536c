"""The NumPy restatement of the weight layouts (tests/pack_ref.py) against what each layout is FOR: the reference's own operations on the
unpacked weights.  tests/test_gpu_pack.py then holds the device equal to the restatement, bit for bit."""
import numpy as np
import torch
import torch.nn.functional as F

import pack_ref as pr


def _w(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def test_conv_is_the_hwio_permutation():
    for O, I, K in ((24, 20, 3), (4, 4, 1), (5, 3, 5)):
        w = _w(1, O, I, K, K)
        got = pr.pack(pr.PACK_CONV, (O, I, K * K), w.numpy())
        assert np.array_equal(got, w.permute(2, 3, 1, 0).reshape(-1).numpy())
        assert got.size == pr.dst_floats(pr.PACK_CONV, (O, I, K * K))


def test_space_to_depth_is_the_rearrangement_then_a_1x1_conv():
    O, C, B, H, W = 8, 4, 2, 6, 4
    w = _w(2, O, 4 * C).double()
    x = _w(3, B, C, H, W).double()
    # Rearrange('b c (h p1) (w p2) -> b (c p1 p2) h w', p1=2, p2=2), then Conv2d(4C, O, 1)
    r = x.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 3, 5, 2, 4).reshape(B, 4 * C, H // 2, W // 2)
    ref = F.conv2d(r, w.reshape(O, 4 * C, 1, 1))
    p = torch.from_numpy(pr.pack(pr.PACK_S2D, (O, C), w.float().numpy())).double().reshape(2, 2, C, O)      # [p1][p2][c][o]
    assert (F.conv2d(x, p.permute(3, 2, 0, 1), stride=2) - ref).abs().max() < 1e-12


def test_padded_conv_is_the_conv_layout_inside_exact_zeros():
    O, I, KK, Op, Ip = 3, 3, 9, 4, 4
    w = _w(4, O, I, KK)
    got = pr.pack(pr.PACK_CONV_PAD, (O, I, KK, Op, Ip), w.numpy()).reshape(KK, Ip, Op)
    assert np.array_equal(got[:, :I, :O].reshape(-1), pr.pack(pr.PACK_CONV, (O, I, KK), w.numpy()))
    mask = np.ones_like(got, dtype=bool)
    mask[:, :I, :O] = False
    assert np.array_equal(got[mask].view(np.uint32), np.zeros(int(mask.sum()), np.uint32))                   # +0, bit for bit


def test_data_gradient_operand_as_a_forward_conv_gives_conv2d_input():
    for O, I, KS, ci0, nci in ((8, 12, 3, 4, 8), (5, 6, 1, 0, 6), (4, 7, 5, 2, 3)):
        pad = KS // 2
        w = _w(5, O, I, KS, KS)
        dy = _w(6, 2, O, 6, 5).double()
        ref = torch.nn.grad.conv2d_input((2, I, 6, 5), w.double(), dy, padding=pad)[:, ci0:ci0 + nci]
        p = torch.from_numpy(pr.pack(pr.PACK_DGRAD, (O, I, KS, ci0, nci), w.numpy())).double().reshape(KS, KS, O, nci)   # [ty][tx][cin' = o][cout' = i]
        got = F.conv2d(dy, p.permute(3, 2, 0, 1), padding=KS - 1 - pad)
        assert (got - ref).abs().max() < 1e-12


def test_k_step_quad_holds_every_element_once_at_its_documented_place():
    O, I, KK = 32, 32, 9
    w = _w(7, O, I, KK).numpy()
    got = pr.pack(pr.PACK_CONV_K8, (O, I, KK), w).reshape(KK, I // 8, 2, O, 4)
    for tap, c8, half, o, jj in ((0, 0, 0, 0, 0), (8, 3, 1, 31, 3), (4, 2, 0, 17, 1), (5, 1, 1, 9, 2)):
        assert got[tap, c8, half, o, jj] == w[o, 8 * c8 + 2 * jj + half, tap]
    assert np.array_equal(np.sort(got.reshape(-1)), np.sort(w.reshape(-1)))


def test_split_hi_is_torch_bfloat16_and_hi_plus_lo_is_x_to_2_pow_minus_16():
    x = _w(8, 4096)
    x[:6] = torch.tensor([0.0, -0.0, 1.5, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8)])
    hi, lo = pr.split_bf16(x.numpy())
    assert np.array_equal(hi, x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    assert pr.bf16_to_f32(hi[3:5]).tolist() == [1.0, 1.0 + 2.0 ** -6]                                        # ties go to the even mantissa
    assert lo[2] == 0 and hi[1] == 0x8000
    back = pr.bf16_to_f32(hi).astype(np.float64) + pr.bf16_to_f32(lo).astype(np.float64)
    assert np.all(np.abs(back - x.double().numpy()) <= 2.0 ** -16 * np.abs(x.double().numpy()))


def test_split_conv_is_the_conv_layout_in_channel_octets():
    O, I, KK, Ipad = 8, 20, 9, 32
    w = _w(9, O, I, KK).numpy()
    got = pr.pack(pr.PACK_CONV_B3, (O, I, KK, Ipad), w).view(np.uint16).reshape(2, KK, Ipad // 8, O, 8)
    hi, lo = pr.split_bf16(w)
    for tap, ci, o in ((0, 0, 0), (8, 19, 7), (3, 9, 4)):
        assert got[0, tap, ci // 8, o, ci % 8] == hi[o, ci, tap] and got[1, tap, ci // 8, o, ci % 8] == lo[o, ci, tap]
    assert not got[:, :, 2, :, 4:].any() and not got[:, :, 3].any()                                          # channels 20..31


def test_four_parity_kernels_equal_nearest_upsampling_plus_conv3x3():
    O, I = 8, 20
    w = _w(10, O, I, 3, 3)
    x = _w(11, 2, I, 4, 6).double()
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w.double(), padding=1)
    f = torch.from_numpy(pr.pack(pr.PACK_UP4, (O, I), w.numpy())).reshape(4, 2, 2, I, O)                     # [parity][ty][tx][i][o]
    y = torch.zeros_like(ref)
    for a in range(2):
        for b in range(2):
            y[:, :, a::2, b::2] = F.conv2d(F.pad(x, (1 - b, b, 1 - a, a)), f[2 * a + b].permute(3, 2, 0, 1).double())
    assert (y - ref).abs().max() < 1e-5 * ref.abs().max()                                                    # the folded taps are fp32 sums
    # the split form holds the same sums, split, per parity
    got = pr.pack(pr.PACK_UP4_B3, (O, I, 32), w.numpy()).view(np.uint16).reshape(4, 2, 4, 4, O, 8)
    hi, lo = pr.split_bf16(f.reshape(4, 4, I, O).numpy())
    for par, tap, ci, o in ((0, 0, 0, 0), (3, 3, 19, 7), (2, 1, 8, 3)):
        assert got[par, 0, tap, ci // 8, o, ci % 8] == hi[par, tap, ci, o] and got[par, 1, tap, ci // 8, o, ci % 8] == lo[par, tap, ci, o]


def test_slices_leave_the_rest_of_the_buffer_alone():
    R, Cc, ld, col0 = 12, 8, 20, 5
    src = _w(12, R, Cc).numpy()
    buf = np.full(Cc * ld, -7.0, np.float32)
    got = pr.pack(pr.PACK_TRANSPOSE, (R, Cc, ld, col0), src, dst=buf).reshape(Cc, ld)
    assert np.array_equal(got[:, col0:col0 + R], src.T) and np.all(got[:, :col0] == -7.0) and np.all(got[:, col0 + R:] == -7.0)
    got = pr.pack(pr.PACK_COPY, (5,), src.reshape(-1)[:5], dst=np.full(8, -7.0, np.float32))
    assert np.array_equal(got[:5], src.reshape(-1)[:5]) and np.all(got[5:] == -7.0)
