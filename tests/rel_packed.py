"""Host model of the packed sparse operand of the relation tables (numpy only; include/gnnrag.h:
gnnrag_rel_transform_packed, csrc/rel_transform.hip).

Per relation row 1408 bytes: the three bf16 planes of the exact 3-way split of |T[r, :]| (224 values each, zeros from D
on), then 64 index bytes.  The index byte of the four columns 4q .. 4q+3 is 0x88 | s0 | s1 << 2 | s2 << 4 | s3 << 6 with
s = (T[r, k] < 0), stored at byte (q % 8 / 2) * 16 + (q / 8) * 2 + q % 2 of the 64 (the order in which the lanes of
k_tables_vq read their 16-bit index words); the eight bytes without columns are 0.
"""
import numpy as np

import b3_probe as bp

HALF = 224                   # values per plane of a row
PLANE_B = 2 * HALF           # bytes per plane
IDX_B = 3 * PLANE_B          # offset of the index bytes
ROW_B = IDX_B + 64           # 1408
NQ = HALF // 4               # groups of four columns (56)


def planes3(x):
    """bp.split3 without its exactness assertion (a value below the smallest bf16 has three empty planes): the bf16 bit
    patterns (uint16) of hi, mid, lo."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = bp.bf16(x)
    r = (x - hi).astype(np.float32)
    mid = bp.bf16(r)
    lo = bp.bf16((r - mid).astype(np.float32))
    return [(p.view(np.uint32) >> np.uint32(16)).astype(np.uint16) for p in (hi, mid, lo)]


def index_pos(q):
    """Byte of group q inside the 64 index bytes."""
    q = np.asarray(q)
    return (q % 8 // 2) * 16 + (q // 8) * 2 + q % 2


def index_byte(s):
    """s [..., 4] bool (T < 0 of four consecutive k) -> the index byte."""
    s = np.asarray(s).astype(np.uint8)
    return (np.uint8(0x88) | s[..., 0] | (s[..., 1] << 2) | (s[..., 2] << 4) | (s[..., 3] << 6)).astype(np.uint8)


def pack(T):
    """T [..., R1, D] fp32 -> [..., R1, 1408] uint8."""
    T = np.ascontiguousarray(T, dtype=np.float32)
    D = T.shape[-1]
    assert D % 4 == 0 and D <= HALF
    out = np.zeros(T.shape[:-1] + (ROW_B,), dtype=np.uint8)
    for p, bits in enumerate(planes3(np.abs(T))):
        out[..., p * PLANE_B:p * PLANE_B + 2 * D] = np.ascontiguousarray(bits.astype("<u2")).view(np.uint8).reshape(T.shape[:-1] + (2 * D,))
    neg = np.zeros(T.shape[:-1] + (HALF,), dtype=bool)
    neg[..., :D] = T < 0                                       # (-0.0 is not below zero)
    out[..., IDX_B + index_pos(np.arange(NQ))] = index_byte(neg.reshape(T.shape[:-1] + (NQ, 4)))
    return out


def unpack(packed, D):
    """The inverse: (|T| as the three planes' fp32 values [3, ..., R1, D], T < 0 [..., R1, D])."""
    packed = np.asarray(packed, dtype=np.uint8)
    planes = []
    for p in range(3):
        bits = np.ascontiguousarray(packed[..., p * PLANE_B:(p + 1) * PLANE_B]).view("<u2").astype(np.uint32)
        planes.append((bits << np.uint32(16)).view(np.float32)[..., :D])
    ib = packed[..., IDX_B + index_pos(np.arange(NQ))]
    neg = np.stack([(ib >> (2 * e)) & 1 for e in range(4)], -1).reshape(packed.shape[:-1] + (HALF,)).astype(bool)
    return np.stack(planes), neg[..., :D]
