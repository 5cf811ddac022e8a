"""The packed sparse operand of the relation tables on the host (tests/rel_packed.py): the packer and its inverse round-trip,
and the index byte is the one vq_compress (csrc/tables_b3.hip) builds from the public planes - for every sign pattern."""
import itertools

import numpy as np

import b3_probe as bp
import rel_packed as rp


def _vq_compress_index(neg8):
    """The rule of vq_compress, restated: the lane's 8 compressed values sit in 4 dwords, value 2 i in the low and value
    2 i + 1 in the high half of dword i; ix = 0x8888 | for every i: (low is negative) | (high is negative) << 2, at 4 i."""
    ix = 0x8888
    for i in range(4):
        ix |= (int(neg8[2 * i]) | (int(neg8[2 * i + 1]) << 2)) << (4 * i)
    return ix


def test_index_byte_is_the_rule_of_vq_compress():
    pats = list(itertools.product((False, True), repeat=4))
    assert len(pats) == 16
    for lo4 in pats:
        for hi4 in pats:
            word = int(rp.index_byte(np.array(lo4))) | (int(rp.index_byte(np.array(hi4))) << 8)      # little endian
            assert word == _vq_compress_index(lo4 + hi4), (lo4, hi4)
            # what the instruction reads: value e at bits 2 e; the first of a (+, -) pair pair at position 0 / 1 of its
            # group of four, the second at 2 / 3 - always ascending
            for e, n in enumerate(lo4 + hi4):
                assert (word >> (2 * e)) & 3 == 2 * (e & 1) + int(n)


def test_index_positions_are_a_permutation_in_lane_order():
    pos = rp.index_pos(np.arange(64))
    assert sorted(pos.tolist()) == list(range(64))
    for blk in range(7):
        for fg in range(4):                                    # the lane's two bytes are one aligned 16-bit word
            q = 8 * blk + 2 * fg
            assert rp.index_pos(q) == fg * 16 + blk * 2 and rp.index_pos(q + 1) == fg * 16 + blk * 2 + 1
    assert rp.ROW_B == 1408 and rp.ROW_B % 16 == 0 and rp.PLANE_B % 16 == 0


def _values(rng, shape):
    T = rng.standard_normal(shape).astype(np.float32)
    u = rng.random(shape)
    T[u < 0.05] = 0.0
    T[(u >= 0.05) & (u < 0.10)] = -0.0
    T[(u >= 0.10) & (u < 0.13)] = np.float32(-1e-41)           # negative, three empty planes
    T[(u >= 0.13) & (u < 0.15)] = np.float32(1e-41)
    return T


def test_pack_round_trip():
    rng = np.random.default_rng(3)
    for D in (200, 208, 224):
        T = _values(rng, (2, 2, 37, D))
        pk = rp.pack(T)
        assert pk.shape == (2, 2, 37, rp.ROW_B) and pk.dtype == np.uint8
        planes, neg = rp.unpack(pk, D)
        assert np.array_equal(neg, T < 0)
        a = np.abs(T)
        big = a >= np.float32(2.0 ** -100)                     # three bf16 planes hold these exactly
        tot = planes[0].astype(np.float64) + planes[1].astype(np.float64) + planes[2].astype(np.float64)
        assert np.array_equal(tot[big], a[big].astype(np.float64))
        assert (tot[a == 0] == 0).all() and (tot[a == np.float32(1e-41)] == 0).all()
        assert np.array_equal(np.where(neg, -tot, tot)[big], T[big].astype(np.float64))
        for p, want in enumerate(bp.split3(np.where(big, a, 0))):
            assert np.array_equal(planes[p][big], want[big])
        # padding: zero planes behind D, "all +" index bytes behind D, zeros where no column stands
        for p in range(3):
            assert (pk[..., p * rp.PLANE_B + 2 * D:(p + 1) * rp.PLANE_B] == 0).all()
        assert (pk[..., rp.IDX_B + rp.index_pos(np.arange(D // 4, rp.NQ))] == 0x88).all()
        assert (pk[..., rp.IDX_B + rp.index_pos(np.arange(rp.NQ, 64))] == 0).all()
        assert np.array_equal(rp.pack(T), pk)


def test_pack_is_the_or_of_the_public_planes():
    """planes of |T| = plane of relu(T) OR plane of relu(-T), bit for bit (the half that is zero holds 0x0000)."""
    rng = np.random.default_rng(4)
    T = _values(rng, (37, 200))
    pk = rp.pack(T)
    pos, neg = rp.planes3(np.maximum(T, 0) + np.float32(0)), rp.planes3(np.maximum(-T, 0) + np.float32(0))
    for p in range(3):
        got = np.ascontiguousarray(pk[:, p * rp.PLANE_B:p * rp.PLANE_B + 400]).view("<u2")
        assert np.array_equal(got, pos[p] | neg[p])
