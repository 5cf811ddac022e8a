"""Host side of the split-K linear and of the encoder's switch onto it (CPU, no GPU): header, binding and exports of the five
entry points, the plan as a function of (K, Nout) alone, forced values, workspace sizes, every argument rule (answered before
a device is touched) and the two host decisions of ``lm_encoder``: the environment switch and the row bound."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_UNSUPPORTED, E_BADARG = -2, -1
NEW = ("gnnrag_linear_splitk_plan", "gnnrag_linear_splitk_workspace_bytes", "gnnrag_linear_splitk",
       "gnnrag_bert_splitk_workspace_bytes", "gnnrag_bert_encode_splitk")
BIAS, GELU, ADD_LN = 0, 1, 2
OK, ODD = 0x10000, 0x10004                      # stand-in addresses: nothing is dereferenced before the answer


@pytest.fixture(scope="module")
def lib():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    return _lib.load()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gnnrag.h")).read(), flags=re.S)


def _plan(lib, M, K, Nout, splits=0):
    from gnnrag_amd import _lib
    p = _lib.SplitkPlanStruct()
    rc = lib.gnnrag_linear_splitk_plan(M, K, Nout, splits, C.byref(p))
    return rc, (p.splits, p.k_chunk, p.launches)


# -- header, binding, exports ------------------------------------------------------------------------------------------

def test_header_binding_and_exports_agree(lib):
    from gnnrag_amd import _lib, build, ops
    src = _header()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src), "not declared: " + n
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert lib.gnnrag_abi_version() == _lib.ABI_VERSION == 16
    # the struct: 8 int32; the constants of the header are the binding's
    assert "int32_t splits, k_chunk, launches, reserved[5];" in src
    assert C.sizeof(_lib.SplitkPlanStruct) == 32
    consts = dict(re.findall(r"#define (GNNRAG_SPLITK_\w+)\s+(\d+)", src))
    assert {k: int(consts["GNNRAG_SPLITK_EPI_" + k.upper()]) for k in _lib.SPLITK_EPI} == _lib.SPLITK_EPI
    assert int(consts["GNNRAG_SPLITK_MAX_SPLITS"]) == _lib.SPLITK_MAX_SPLITS
    # the encoder entry takes the arguments of gnnrag_bert_encode_ex
    assert _lib.SIGNATURES["gnnrag_bert_encode_splitk"] == _lib.SIGNATURES["gnnrag_bert_encode_ex"]
    assert _lib.SIGNATURES["gnnrag_bert_splitk_workspace_bytes"] == _lib.SIGNATURES["gnnrag_bert_workspace_bytes"]
    assert len(_lib.SIGNATURES["gnnrag_linear_splitk"][1]) == 16
    assert "linear_splitk.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "linear_splitk.hip"))
    for n in ("linear_splitk_plan", "linear_splitk"):
        assert callable(getattr(ops, n))
    assert ops.SplitkPlan._fields == ("splits", "k_chunk", "launches")


# -- the plan ---------------------------------------------------------------------------------------------------------

SHAPES = [(4, 4), (36, 60), (100, 200), (384, 1152), (384, 384), (1536, 384), (768, 2304), (768, 768), (768, 3072),
          (3072, 768), (4096, 4096), (1 << 20, 4), (8, 1 << 20)]


@pytest.mark.parametrize("K,Nout", SHAPES)
def test_the_automatic_plan_reads_k_and_nout_only(lib, K, Nout):
    from gnnrag_amd import _lib, ops
    rc, one = _plan(lib, 1, K, Nout)
    assert rc == 0
    for M in (12, 16, 17, 1280, 100000, (1 << 31) - 1):
        assert _plan(lib, M, K, Nout) == (0, one)
    S, chunk, launches = one
    print("K=%d Nout=%d: splits %d, k_chunk %d, launches %d" % (K, Nout, S, chunk, launches))
    assert 1 <= S <= _lib.SPLITK_MAX_SPLITS and chunk % 4 == 0 and launches == 2
    assert S * chunk >= K and (S - 1) * chunk < K
    assert ops.linear_splitk_plan(100000, K, Nout) == ops.SplitkPlan(*one)


@pytest.mark.parametrize("K", [4, 36, 100, 3072])
def test_forced_values_are_honoured_or_refused(lib, K):
    from gnnrag_amd import _lib
    legal = []
    for s in range(1, _lib.SPLITK_MAX_SPLITS + 2):
        rc, (S, chunk, _) = _plan(lib, 7, K, 64, s)
        want = -(-(-(-K // s)) // 4) * 4        # ceil(K / s) rounded up to a multiple of 4
        if s <= _lib.SPLITK_MAX_SPLITS and (s - 1) * want < K:
            assert rc == 0 and (S, chunk) == (s, want), (s, rc, S, chunk)
            assert S * chunk >= K and (S - 1) * chunk < K
            assert _plan(lib, 100000, K, 64, s) == (0, (S, chunk, 2))
            legal.append(s)
        else:
            assert rc == E_UNSUPPORTED, (s, rc)
            assert lib.gnnrag_linear_splitk_workspace_bytes(7, K, 64, s) == 0
    print("K=%d: %d legal forced values, largest %d" % (K, len(legal), legal[-1]))
    assert legal[0] == 1 and legal[-1] == min(K // 4, _lib.SPLITK_MAX_SPLITS)
    assert {4: [1], 36: [1, 2, 3, 5, 9]}.get(K, legal) == legal      # 4 x 12 would leave the fourth chunk empty


def test_workspace_bytes(lib):
    f = lib.gnnrag_linear_splitk_workspace_bytes
    for M, K, Nout, s in ((17, 100, 68, 3), (1, 4, 4, 1), (12, 3072, 768, 0), (37, 384, 200, 96), (100000, 768, 768, 0),
                          ((1 << 31) - 1, 64, 64, 4)):
        rc, (S, _, _) = _plan(lib, M, K, Nout, s)
        assert rc == 0 and (s == 0 or S == s)
        raw = S * M * Nout * 4
        assert f(M, K, Nout, s) == (raw + 255) // 256 * 256     # the header: rounded up to a multiple of 256
    assert f(0, 4, 4, 0) == 0 and f(1, 6, 4, 0) == 0 and f(1, 4, 6, 0) == 0 and f(1, 4, 4, -1) == 0
    # the encoder's: qkv, ctx, ffn (each from a 256-byte boundary) and the largest of the four products' partials
    g = lib.gnnrag_bert_splitk_workspace_bytes
    for B, T, H, I in ((1, 12, 384, 1536), (3, 9, 768, 3072), (5, 20, 64, 128)):
        M = B * T
        up = lambda n: (n + 255) // 256 * 256
        part = max(f(M, H, 3 * H, 0), f(M, H, H, 0), f(M, H, I, 0), f(M, I, H, 0))
        assert g(B, T, H, I) == up(M * 3 * H * 4) + up(M * H * 4) + up(M * I * 4) + part
    assert g(0, 9, 384, 1536) == 0 and g(1, 9, 384, 1534) == 0 and g(1, 9, 382, 1536) == 0


# -- the argument rules, in the header's order ------------------------------------------------------------------------------

def _call(lib, M=17, K=100, Nout=68, splits=3, epi=BIAS, A=OK, W=OK, bias=OK, add=None, g=None, b=None, Cp=OK, ws=OK,
          ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.gnnrag_linear_splitk_workspace_bytes(M, K, Nout, splits)
    return lib.gnnrag_linear_splitk(A, M, K, W, bias, epi, add, g, b, 1e-12, Cp, Nout, splits, ws, ws_bytes, None)


def test_argument_rules_without_a_device(lib):
    from gnnrag_amd import _lib
    none = dict(A=None, W=None, bias=None, Cp=None, ws=None)
    # sizes, the epilogue, a negative splits: BADARG before anything else
    for kw in (dict(M=0), dict(M=-1), dict(K=0), dict(Nout=0), dict(Nout=-4), dict(splits=-1), dict(epi=3), dict(epi=-1)):
        assert _call(lib, ws_bytes=1 << 30, **none, **kw) == E_BADARG, kw
    # the shape rules with NULL everywhere: UNSUPPORTED; the same call with a legal shape: BADARG (the pointers' turn)
    assert _call(lib, **none) == E_BADARG
    for kw in (dict(K=102), dict(Nout=66), dict(splits=_lib.SPLITK_MAX_SPLITS + 1, K=4096), dict(splits=7, K=36),
               dict(splits=2, K=4), dict(M=1 << 31)):
        assert _call(lib, ws_bytes=1 << 40, **none, **kw) == E_UNSUPPORTED, kw
    need = lib.gnnrag_linear_splitk_workspace_bytes(17, 100, 68, 3)
    assert need == (3 * 17 * 68 * 4 + 255) // 256 * 256
    assert _call(lib, ws_bytes=need - 1, **none) == E_UNSUPPORTED
    assert _call(lib, ws_bytes=0, **none) == E_UNSUPPORTED
    # NULL pointers the epilogue needs; bias may be NULL (the alignment rule answers next: ODD)
    for kw in (dict(A=None), dict(W=None), dict(Cp=None), dict(ws=None)):
        assert _call(lib, **kw) == E_BADARG, kw
    assert _call(lib, bias=None, A=ODD) == E_UNSUPPORTED
    full = dict(add=OK, g=OK, b=OK)
    for name in full:
        assert _call(lib, epi=ADD_LN, **{**full, name: None}) == E_BADARG, name
    for epi in (BIAS, GELU):
        assert _call(lib, epi=epi, A=ODD) == E_UNSUPPORTED          # add / ln are not looked at
    # alignment
    for kw in (dict(A=ODD), dict(W=ODD), dict(bias=ODD), dict(Cp=ODD), dict(ws=ODD)):
        assert _call(lib, **kw) == E_UNSUPPORTED, kw
    for name in full:
        assert _call(lib, epi=ADD_LN, **{**full, name: ODD}) == E_UNSUPPORTED, name
    # the plan: the same order, a NULL plan last
    assert lib.gnnrag_linear_splitk_plan(0, 100, 68, 3, None) == E_BADARG
    assert lib.gnnrag_linear_splitk_plan(17, 102, 68, 3, None) == E_UNSUPPORTED
    assert lib.gnnrag_linear_splitk_plan(17, 100, 68, 3, None) == E_BADARG


def _encode(lib, B=2, T=9, H=384, heads=12, I=1536, L=1, max_pos=16, ws_bytes=None, ptr=None, layer_ptr=None, ws=None,
            math=0):
    from gnnrag_amd import _lib
    layers = (_lib.BertLayer * max(L, 1))()
    for l in range(L):
        for n, _ in _lib.BertLayer._fields_:
            setattr(layers[l], n, layer_ptr)
    if ws_bytes is None:
        ws_bytes = lib.gnnrag_bert_splitk_workspace_bytes(B, T, H, I)
    return lib.gnnrag_bert_encode_splitk(ptr, ptr, 64, ptr, max_pos, ptr, -1, None, ptr, ptr, 1e-12, L, layers, B, T, H,
                                         heads, I, ptr, ptr if ws is None else ws, ws_bytes, math, None)


def test_encoder_entry_rules_without_a_device(lib):
    assert _encode(lib) == E_BADARG                                  # a legal shape: the NULL pointers answer
    assert _encode(lib, B=0) == E_BADARG and _encode(lib, math=7) == E_BADARG
    assert _encode(lib, H=192, heads=12) == E_UNSUPPORTED            # dh = 16
    assert _encode(lib, T=129, max_pos=512) == E_UNSUPPORTED
    assert _encode(lib, T=17, max_pos=16) == E_UNSUPPORTED
    assert _encode(lib, I=1534) == E_UNSUPPORTED                     # FFN-out's K % 4
    need = lib.gnnrag_bert_splitk_workspace_bytes(2, 9, 384, 1536)
    assert need > 0
    assert _encode(lib, ws_bytes=need - 1) == E_UNSUPPORTED and _encode(lib, ws_bytes=0) == E_UNSUPPORTED
    assert _encode(lib, L=0, ws_bytes=0) == E_BADARG                 # L = 0 needs none
    assert _encode(lib, L=0, ptr=ODD) == E_UNSUPPORTED
    assert _encode(lib, ptr=OK, layer_ptr=ODD) == E_UNSUPPORTED
    assert _encode(lib, ptr=OK, layer_ptr=OK, ws=ODD) == E_UNSUPPORTED
    assert _encode(lib, ptr=OK, layer_ptr=None) == E_BADARG


# -- the switch and the row bound -----------------------------------------------------------------------------------------

def test_env_parsing_and_the_row_bound(monkeypatch):
    from gnnrag_amd.modules.question_encoding import lm_encoder as lm
    monkeypatch.delenv("GNNRAG_HIP_LM_SPLITK", raising=False)
    assert lm.SPLITK_DEFAULT == "0" and not lm.splitk_enabled()      # ships off
    for v, want in (("0", False), ("", False), ("1", True), ("2", True), ("on", True)):
        monkeypatch.setenv("GNNRAG_HIP_LM_SPLITK", v)
        assert lm.splitk_enabled() is want, v                        # read at every call
    monkeypatch.delenv("GNNRAG_HIP_LM_SPLITK")
    assert not lm.splitk_enabled()
    assert lm.DEFAULT_ON == ("BertModel",)                           # unchanged
    R = lm.SPLITK_MAX_ROWS
    assert isinstance(R, int) and 12 <= R < 1280
    assert lm.splitk_rows_ok(1, 12) and lm.splitk_rows_ok(1, R) and lm.splitk_rows_ok(R, 1)
    assert not lm.splitk_rows_ok(1, R + 1) and not lm.splitk_rows_ok(R // 2 + 1, 2) and not lm.splitk_rows_ok(64, 20)
    assert not lm.splitk_rows_ok(0, 12)


def test_patch_counts_split_k_calls_from_zero():
    pytest.importorskip("transformers")
    import bert_oracle as bo
    from gnnrag_amd.modules.question_encoding.lm_encoder import patch_lm_encoder

    class Holder:
        node_encoder = bo.make_model(bo.config(H=64, heads=2, I=128, L=1, vocab=50, max_pos=16), seed=5)[0]

    patch_lm_encoder(Holder)
    p = Holder.node_encoder._gnnrag_lm_patch
    assert (p.hip_calls, p.hip_train_calls, p.hip_splitk_calls) == (0, 0, 0)
