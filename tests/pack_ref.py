"""NumPy restatement of the ten weight layouts (flocoder_amd/csrc/common.h `PackKind`), written from the formulae documented there.

``pack(kind, dims, src)`` returns the destination as a flat float32 array (the two split-bf16 layouts as the float32 view of their 16-bit
values); ``dst_floats(kind, dims)`` its length.  ``dims`` are the arguments of the kind's constructor (`pack_job_*`), in order.  PACK_TRANSPOSE
and PACK_COPY write into a slice of a buffer: they take ``dst`` (the buffer before the job) and return it with the slice filled.

The two summing layouts add in float32 in the kernel's stated order (ky outer, kx inner, starting from 0), the split is the kernel's
integer round-to-nearest-even; everything else is a permutation, so the comparison with the device needs no tolerance.
"""
import numpy as np

(PACK_CONV, PACK_S2D, PACK_TRANSPOSE, PACK_COPY, PACK_CONV_PAD, PACK_DGRAD, PACK_CONV_K8, PACK_CONV_B3, PACK_UP4, PACK_UP4_B3) = range(10)
N_KINDS = 10

# rows ky (columns kx alike) of the 3x3 kernel that land on row ty of the 2x2 window of output parity a: FOLD[a][ty]
FOLD = (((0,), (1, 2)), ((0, 1), (2,)))


def bf16_rne(x):
    """float32 array -> the 16 bits of bfloat16(x), round to nearest even, by the integer rule u + 0x7fff + ((u >> 16) & 1)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff).astype(np.uint16)


def bf16_to_f32(h):
    return (h.astype(np.uint32) << 16).view(np.float32)


def split_bf16(x):
    """x = hi + lo: hi = bf16(x), lo = bf16(x - hi), the subtraction in float32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = bf16_rne(x)
    return hi, bf16_rne(x - bf16_to_f32(hi))


def _as_f32(h16):
    return np.ascontiguousarray(h16).reshape(-1).view(np.float32)


def _chan8(w_tio, ipad):
    """[tap][I][O] -> [tap][Ipad/8][O][8], channels beyond I zero."""
    kk, i, o = w_tio.shape
    p = np.zeros((kk, ipad, o), np.float32)
    p[:, :i] = w_tio
    return p.reshape(kk, ipad // 8, 8, o).transpose(0, 1, 3, 2)


def _fold(w):
    """[O][I][3][3] -> [parity 2a + b][tap 2ty + tx][I][O], float32 sums in the order ky outer, kx inner, from 0."""
    o, i = w.shape[:2]
    out = np.zeros((4, 4, i, o), np.float32)
    for a in range(2):
        for b in range(2):
            for ty in range(2):
                for tx in range(2):
                    acc = np.zeros((o, i), np.float32)
                    for ky in FOLD[a][ty]:
                        for kx in FOLD[b][tx]:
                            acc = (acc + w[:, :, ky, kx]).astype(np.float32)
                    out[2 * a + b, 2 * ty + tx] = acc.T
    return out


def dst_floats(kind, dims):
    d = list(dims) + [0] * 5
    return {PACK_CONV: d[0] * d[1] * d[2], PACK_S2D: 4 * d[0] * d[1], PACK_TRANSPOSE: d[1] * d[2], PACK_COPY: d[0],
            PACK_CONV_PAD: d[3] * d[4] * d[2], PACK_DGRAD: d[0] * d[4] * d[2] * d[2], PACK_CONV_K8: d[0] * d[1] * d[2],
            PACK_CONV_B3: d[0] * d[3] * d[2], PACK_UP4: 16 * d[0] * d[1], PACK_UP4_B3: 16 * d[0] * d[2]}[kind]


def src_floats(kind, dims):
    d = list(dims) + [0] * 5
    return {PACK_S2D: 4 * d[0] * d[1], PACK_TRANSPOSE: d[0] * d[1], PACK_COPY: d[0], PACK_DGRAD: d[0] * d[1] * d[2] * d[2],
            PACK_UP4: 9 * d[0] * d[1], PACK_UP4_B3: 9 * d[0] * d[1]}.get(kind, d[0] * d[1] * d[2])


def pack(kind, dims, src, dst=None):
    src = np.ascontiguousarray(src, dtype=np.float32).reshape(-1)
    if kind == PACK_CONV:                # dst[tap][ci][o] = w[o][ci][tap]
        O, I, KK = dims
        return src.reshape(O, I, KK).transpose(2, 1, 0).reshape(-1).copy()
    if kind == PACK_S2D:                 # dst[tap = 2 p1 + p2][c][o] = w[o][4 c + tap]
        O, C = dims
        return src.reshape(O, C, 4).transpose(2, 1, 0).reshape(-1).copy()
    if kind == PACK_TRANSPOSE:           # dst[c * ld + col0 + r] = src[r][c]
        R, Cc, ld, col0 = dims
        out = dst.copy().reshape(Cc, ld)
        out[:, col0:col0 + R] = src.reshape(R, Cc).T
        return out.reshape(-1)
    if kind == PACK_COPY:
        out = dst.copy()
        out[:dims[0]] = src
        return out
    if kind == PACK_CONV_PAD:            # dst[tap][ci][o] over [KK][Ipad][Opad], zero where o >= O or ci >= I
        O, I, KK, Opad, Ipad = dims
        out = np.zeros((KK, Ipad, Opad), np.float32)
        out[:, :I, :O] = src.reshape(O, I, KK).transpose(2, 1, 0)
        return out.reshape(-1)
    if kind == PACK_DGRAD:               # dst[(KS-1-ky) KS + (KS-1-kx)][o][i - ci0] = w[o][i][ky][kx]
        O, I, KS, ci0, nci = dims
        w = src.reshape(O, I, KS, KS)[:, ci0:ci0 + nci, ::-1, ::-1]
        return w.transpose(2, 3, 0, 1).reshape(-1).copy()
    if kind == PACK_CONV_K8:             # dst[tap][c8][half][o][jj] = w[o][8 c8 + 2 jj + half][tap]
        O, I, KK = dims
        return src.reshape(O, I // 8, 4, 2, KK).transpose(4, 1, 3, 0, 2).reshape(-1).copy()
    if kind == PACK_CONV_B3:             # hi parts, then lo parts, each [tap][c8][o][jj] 16-bit, ci = 8 c8 + jj
        O, I, KK, Ipad = dims
        hi, lo = split_bf16(_chan8(src.reshape(O, I, KK).transpose(2, 1, 0), Ipad))
        return _as_f32(np.stack([hi, lo]))
    if kind == PACK_UP4:
        O, I = dims
        return _fold(src.reshape(O, I, 3, 3)).reshape(-1)
    if kind == PACK_UP4_B3:              # [parity][hi | lo][tap][c8][o][jj] 16-bit
        O, I, Ipad = dims
        f = _fold(src.reshape(O, I, 3, 3))
        parts = [np.stack(split_bf16(_chan8(f[p], Ipad))) for p in range(4)]
        return _as_f32(np.stack(parts))
    raise ValueError(f"no such layout: {kind}")
