"""Host-only proof that the dense case table (tests/dense_cases.py) reaches what it claims, and pins of the dense
dispatch thresholds - through ``ops.dense_form`` (``gnnrag_dense_form``: the launchers' own decision function, no HIP
call), so none of this needs a GPU.  Moving kSkinnyMaxM, the MT = 2 bound or the NW rule fails a test here."""
import itertools

import pytest

import dense_cases as dc


@pytest.fixture(scope="module")
def ops():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib, ops
    _lib.load()
    return ops


def _query(ops, c, block=0):
    return ops.dense_form(c.entry, c.M, c.K, c.N, math=c.math, add_rows=dc.add_rows(c), misaligned=c.mis, block=block)


def _kform(f):
    return dc.KForm(f.epi, f.nt, f.mt, f.nw, f.v4, f.math, f.v4out, f.n0)


def test_constants_match_the_binding(ops):
    assert (dc.MIS_A, dc.MIS_W, dc.MIS_C, dc.MIS_ADD, dc.MIS_A1) == (
        ops.DENSE_MISALIGNED_A, ops.DENSE_MISALIGNED_W, ops.DENSE_MISALIGNED_C, ops.DENSE_MISALIGNED_ADD,
        ops.DENSE_MISALIGNED_A1)
    assert (dc.SKINNY, dc.KTILED, dc.WRES, dc.UPDATE_SKINNY, dc.UPDATE_B3) == (
        ops.DENSE_SKINNY, ops.DENSE_KTILED, ops.DENSE_WRES, ops.DENSE_UPDATE_SKINNY, ops.DENSE_UPDATE_B3)
    assert dc.MATHS == (ops.MATH_FP32, ops.MATH_BF16X3, ops.MATH_MIXED)


@pytest.mark.parametrize("c", dc.CASES, ids=dc.case_id)
def test_every_case_runs_the_form_it_names(ops, c):
    f = _query(ops, c)
    assert f.family == c.family == f.block_family, (f, c)
    if c.family != dc.KTILED:
        return
    per_call = len(c.forms)
    assert f.launches == per_call * (2 if c.entry == "linear_pair" else 1)
    for blk, want in enumerate(c.forms):
        assert _kform(_query(ops, c, blk)) == want, (blk, c)
    from gnnrag_amd import _lib
    with pytest.raises(_lib.GnnragError) as err:
        _query(ops, c, per_call)                 # a block the call does not launch
    assert err.value.code == -1                  # GNNRAG_E_BADARG


def _forms_of(epi):
    return {(f.nt, f.mt, f.nw, f.v4, f.math) for c in dc.CASES for f in c.forms if f.epi == epi}


def test_table_reaches_all_54_ktiled_instantiations():
    """EPI_LINEAR and EPI_UPDATE (AMODE_PLAIN), NT in {4, 8, 13} x (MT, NW) in {(1,4), (1,8), (2,4)} x
    (V4, MATH) in {(1,1), (1,0), (0,0)}: every one is reached by a case (and test_every_case_runs_the_form_it_names
    holds each case to its form), none is unreachable."""
    want = {(nt, mt, nw, v4, m) for nt in (4, 8, 13) for (mt, nw) in ((1, 4), (1, 8), (2, 4))
            for (v4, m) in ((1, 1), (1, 0), (0, 0))}
    assert len(want) == 27
    for epi in (dc.EPI_LINEAR, dc.EPI_UPDATE):
        got = _forms_of(epi)
        assert got == want, (epi, sorted(want - got), sorted(got - want))


def test_no_other_ktiled_form_exists(ops):
    """(V4, MATH) = (0, 1) has no instantiation and (MT, NW) = (2, 8) neither: a sweep over sizes, math modes and
    alignments through the decision function never names one."""
    seen = set()
    rows = (1, 71, 16384, 16385, 32768, 32769, 65536, 65537, 98304, 98305, 130944, 130945, 300000)
    for M, K, Nout, math, mis in itertools.product(rows, (4, 30, 1000), (8, 72, 136, 1000), dc.MATHS, (0, 1, 2, 4)):
        forms = [ops.dense_form("linear", M, K, Nout, math=math, misaligned=mis)]
        if Nout <= 208:
            forms.append(ops.dense_form("update_score", M, Nout, 1, math=math, misaligned=mis))
        for f in forms:
            if f.block_family == ops.DENSE_KTILED:
                seen.add((f.nt, f.mt, f.nw, f.v4, f.math))
    assert all((mt, nw) in ((1, 4), (1, 8), (2, 4)) for (_, mt, nw, _, _) in seen)
    assert all((v4, m) in ((1, 1), (1, 0), (0, 0)) for (_, _, _, v4, m) in seen)
    assert {nt for (nt, _, _, _, _) in seen} == {4, 8, 13}


@pytest.mark.parametrize("epi", [dc.EPI_LINEAR, dc.EPI_UPDATE])
def test_runtime_edges_occur_per_epi(epi):
    """The epilogue's runtime switches, each at least once per EPI: the scalar epilogue next to the float4 one; a
    ragged last row tile (every row class is 7 rows past a tile); a k tail (K % 32 != 0) and K < 32; `add` present and
    absent; and for EPI_LINEAR n0 > 0, add_rows in {M, M - 1, 1}, no bias, relu on and off."""
    cs = [c for c in dc.CASES if c.family == dc.KTILED and c.forms[0].epi == epi]
    fs = [f for c in cs for f in c.forms]
    assert {f.v4out for f in fs} == {0, 1}
    assert all(c.M % 128 == 7 or c.M in (71, 8191) for c in cs)
    kk = {(c.K if epi == dc.EPI_LINEAR else (c.K if c.entry == "update_score_fused" else (2 * c.N + 1) * c.K)) for c in cs}
    assert any(k % 32 for k in kk) and any(k % 32 == 0 for k in kk) and any(k < 32 for k in kk) and any(k >= 1000 for k in kk)
    assert {c.add is None for c in cs} == {True, False}
    assert {c.mis != 0 for c in cs} == {True, False}
    if epi == dc.EPI_LINEAR:
        assert {c.add for c in cs} == {None, "M", "M-1", "1"}
        assert {c.bias for c in cs} == {True, False} and {c.relu for c in cs} == {True, False}
        assert {f.n0 for f in fs} == {0, 208, 416, 624, 832}
        assert any(f.n0 == 208 and f.nt == 4 for f in fs)                     # the 8-column second block
        assert any(f.n0 > 0 and f.v4out == 0 for f in fs)                     # two blocks, scalar epilogue
        assert {c.N for c in cs} >= {8, 64, 72, 128, 136, 208, 210, 216, 1000}
        assert {c.K for c in cs} >= {4, 30, 32, 36, 200, 1000}
        assert {c.entry for c in cs} == {"linear", "linear_pair"}
    else:
        assert {c.K for c in cs} >= {30, 56, 100, 128, 200, 208} and {c.N for c in cs} == {1, 2}
        assert {c.M for c in cs} >= {71, 16391, 32775, 130951}
        assert {c.entry for c in cs} == {"update_score", "update_score_fused"}


# ---- thresholds ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("math", dc.MATHS)
def test_linear_skinny_bound(ops, math):
    """gnnrag_linear / gnnrag_linear_pair: k_gemm_skinny (exact fp32 whatever the math mode, every column in one
    launch) up to 16384 rows, k_gemm_f32 from 16385."""
    for entry in ("linear", "linear_pair"):
        f = ops.dense_form(entry, 16384, 200, 1000, math=math)
        assert (f.family, f.launches) == (ops.DENSE_SKINNY, 1)
        f = ops.dense_form(entry, 16385, 200, 1000, math=math)
        assert (f.family, f.launches) == (ops.DENSE_KTILED, 5 * (2 if entry == "linear_pair" else 1))
        assert (f.epi, f.nt, f.mt, f.nw, f.math) == (0, 13, 1, 4, int(math != ops.MATH_FP32))


def test_row_tile_rules(ops):
    """MT = 2 (128-row workgroups of 4 waves) from 1024 row tiles of 128, i.e. M = 130945; below, NW = 8 for
    ceil(M / 128) in 257..512 and 768..1023, NW = 4 elsewhere - the same for both epilogues."""
    def mtnw(entry, M):
        f = ops.dense_form(entry, M, 8, 8 if entry == "linear" else 1, math=ops.MATH_FP32)
        assert f.family == ops.DENSE_KTILED
        return (f.mt, f.nw)

    for entry in ("linear", "update_score"):
        assert mtnw(entry, 130944) == (1, 8) and mtnw(entry, 130945) == (2, 4) and mtnw(entry, 1 << 22) == (2, 4)
        for tiles in sorted({129, 130, 200, 256, 257, 258, 300, 511, 512, 513, 600, 767, 768, 769, 900, 1022, 1023}):
            want = (1, 8) if 257 <= tiles <= 512 or 768 <= tiles <= 1023 else (1, 4)
            assert mtnw(entry, tiles * 128) == want, tiles
            assert mtnw(entry, tiles * 128 - 127) == want, tiles
    for tiles in (1, 2, 64, 128):
        assert mtnw("update_score", tiles * 128) == (1, 4)


def test_column_tile_rule(ops):
    for ncol, nt in ((1, 4), (64, 4), (65, 8), (128, 8), (129, 13), (208, 13)):
        assert ops.dense_form("linear", 20000, 8, ncol, math=0).nt == nt
        assert ops.dense_form("update_score", 20000, ncol, 1, math=0).nt == nt
    f = ops.dense_form("linear", 20000, 8, 209, math=0, block=1)
    assert (f.launches, f.n0, f.nt, f.v4out) == (2, 208, 4, 0)


def test_update_fused_families(ops):
    """gnnrag_update_score_fused: k_update_skinny below 4096 rows; from 4096 k_gemm_wres in fp32 and mixed (bf16x3 has
    no W-resident form there and runs k-tiled); from 8192 rows k_update_b3 at D = 200 and 208 in bf16x3 and mixed."""
    q = lambda BN, D, math, **kw: ops.dense_form("update_score_fused", BN, D, 2, math=math, **kw)
    for math in dc.MATHS:
        assert q(4095, 200, math).family == ops.DENSE_UPDATE_SKINNY
        assert q(1, 56, math).family == ops.DENSE_UPDATE_SKINNY
    for math in (ops.MATH_FP32, ops.MATH_MIXED):
        f = q(4096, 200, math)
        assert (f.family, f.nt, f.nc, f.has_add, f.kguard) == (ops.DENSE_WRES, 13, 13, 1, 0)
        f = q(4096, 100, math)
        assert (f.family, f.nt, f.nc, f.has_add, f.kguard) == (ops.DENSE_WRES, 8, 8, 1, 1)
        f = q(4096, 56, math)
        assert (f.family, f.nt, f.nc, f.kguard) == (ops.DENSE_WRES, 4, 4, 0)
    assert q(4096, 200, ops.MATH_BF16X3).family == ops.DENSE_KTILED
    for D in (200, 208):
        for math in (ops.MATH_BF16X3, ops.MATH_MIXED):
            assert q(8192, D, math).family == ops.DENSE_UPDATE_B3
            assert q(8191, D, math).family != ops.DENSE_UPDATE_B3
        assert q(8192, D, ops.MATH_FP32).family != ops.DENSE_UPDATE_B3
    assert q(8192, 192, ops.MATH_MIXED).family == ops.DENSE_WRES          # 12 column tiles: not a k_update_b3 shape
    assert q(8192, 200, ops.MATH_FP32).family == ops.DENSE_WRES
    assert q(8192, 208, ops.MATH_FP32).family == ops.DENSE_KTILED         # the fp32 weight block exceeds a CU's LDS
    # unaligned operands: no W-resident / one-wave kernel, the k-tiled one takes them
    assert q(8192, 200, ops.MATH_MIXED, misaligned=ops.DENSE_MISALIGNED_ADD).family == ops.DENSE_KTILED
    assert q(100, 200, ops.MATH_FP32, misaligned=ops.DENSE_MISALIGNED_A).family == ops.DENSE_KTILED


def test_unfused_update_is_ktiled_at_any_size_and_wide_blocks(ops):
    for BN in (1, 71, 4096, 8192, 200000):
        for math in dc.MATHS:
            f = ops.dense_form("update_score", BN, 200, 2, math=math)
            assert (f.family, f.epi, f.nt) == (ops.DENSE_KTILED, 1, 13)
    # D > 208: EPI_LINEAR column blocks (k_gemm_skinny does them all up to its row bound), then k_score_rows
    f = ops.dense_form("update_score_fused", 300, 256, 1, math=0)
    assert (f.family, f.block_family, f.launches) == (ops.DENSE_WIDE, ops.DENSE_SKINNY, 1)
    f = ops.dense_form("update_score_fused", 20000, 256, 1, math=1, block=1)
    assert (f.family, f.block_family, f.launches, f.epi, f.n0, f.nt) == (ops.DENSE_WIDE, ops.DENSE_KTILED, 2, 0, 208, 4)


def test_bad_arguments(ops):
    from gnnrag_amd import _lib
    lib = _lib.load()
    out = _lib.DenseFormStruct()
    import ctypes
    assert lib.gnnrag_dense_form(0, 10, 8, 8, 0, 0, 0, 0, 0, None) == -1
    assert lib.gnnrag_dense_form(9, 10, 8, 8, 0, 0, 0, 0, 0, ctypes.byref(out)) == -1
    assert lib.gnnrag_dense_form(0, 10, 8, 8, 7, 0, 0, 0, 0, ctypes.byref(out)) == -1
    assert lib.gnnrag_dense_form(0, 0, 8, 8, 0, 0, 0, 0, 0, ctypes.byref(out)) == -1
    assert lib.gnnrag_dense_form(0, 10, 8, 8, 0, 0, 0, 0, 1, ctypes.byref(out)) == -1      # skinny: one launch
