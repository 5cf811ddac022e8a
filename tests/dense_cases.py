"""Case table of the dense-kernel form tests.

One table, two readers: tests/test_dense_forms_host.py proves on the host (``ops.dense_form``, no GPU) that the table
reaches every k_gemm_f32 instantiation the four dense entry points can launch and every runtime edge of its epilogue;
tests/test_gpu_dense_forms.py runs every case on the GPU after asserting the same form.

A case states the kernel form it is there for (``Case.forms``: one tuple per GEMM launch of the call); the expectation
is written from the dispatch rules as documented (row classes, column tiles, loaders), NOT queried from the library -
a moved threshold makes the assertion fail instead of silently moving the case to another kernel.
"""
import collections

MATHS = (0, 1, 2)                  # ops.MATH_FP32, MATH_BF16X3, MATH_MIXED
MIS_A, MIS_W, MIS_C, MIS_ADD, MIS_A1 = 1, 2, 4, 8, 16      # ops.DENSE_MISALIGNED_*
SKINNY, KTILED, WRES, UPDATE_SKINNY, UPDATE_B3 = 1, 2, 3, 4, 5      # ops.DENSE_*
EPI_LINEAR, EPI_UPDATE = 0, 1

# rows -> (MT, NW) of the k-tiled kernel: 128*128+7, 256*128+7, 1023*128+7 (a ragged last tile in each class); 71 rows
# for the unfused update (k-tiled at any size); 8191 = 64 tiles less one row: the fused update at D = 208 one row below
# k_update_b3's bound
ROW_CLASS = {71: (1, 4), 8191: (1, 4), 16391: (1, 4), 32775: (1, 8), 130951: (2, 4)}

# KForm: one k_gemm_f32 launch.  (v4, math) is the loader / MFMA form, v4out the float4 epilogue, n0 the column block.
KForm = collections.namedtuple("KForm", "epi nt mt nw v4 math v4out n0")

# Case: entry point and sizes - (M, K, N) = (M, K, Nout) of the linear entry points, (BN, D, I) of the update ones;
# add: None or the add_rows of the linear entry points ("M", "M-1", "1"); mis: OR of MIS_*;
# family: SKINNY .. UPDATE_B3; forms: KForm per launch (k-tiled cases only).
Case = collections.namedtuple("Case", "entry M K N math add bias relu mis family forms")


def case_id(c):
    return "%s-%dx%dx%d-m%d-add%s-b%d-r%d-mis%d" % (c.entry, c.M, c.K, c.N, c.math, c.add, c.bias, c.relu, c.mis)


def add_rows(c):
    return {None: None, "M": c.M, "M-1": c.M - 1, "1": 1}[c.add]


def _nt(ncol):
    return 4 if ncol <= 64 else 8 if ncol <= 128 else 13


def _linear_forms(M, K, Nout, math, add, mis):
    mt, nw = ROW_CLASS[M]
    v4 = int(K % 4 == 0 and not mis & (MIS_A | MIS_W))
    b3 = int(v4 and math != 0)             # the scalar loaders exist in the exact-fp32 form only
    out = []
    for n0 in range(0, Nout, 208):
        v4out = int(Nout % 4 == 0 and not mis & MIS_C and not (add is not None and mis & MIS_ADD))
        out.append(KForm(EPI_LINEAR, _nt(Nout - n0), mt, nw, v4, b3, v4out, n0))
    return tuple(out)


def _update_forms(BN, D, I, math, mis, fused):
    mt, nw = ROW_CLASS[BN]
    v4 = int(D % 4 == 0 and not mis & (MIS_A | MIS_W | MIS_A1))
    v4out = int(D % 4 == 0 and not mis & MIS_C and not (fused and mis & MIS_ADD))
    return (KForm(EPI_UPDATE, _nt(D), mt, nw, v4, int(v4 and math != 0), v4out, 0),)


# ---- gnnrag_linear above the skinny bound: (M, K, Nout, add, bias, relu, mis), each in all three math modes ----------
# Large K stays with the smallest row class and small K with the largest (float64 reference <= ~2 GFLOP).
_LINEAR = [
    # (MT, NW) = (1, 4)
    (16391, 1000, 64, None, True, False, 0),        # NT 4, the long k loop
    (16391, 200, 128, "M", True, True, 0),          # NT 8
    (16391, 200, 208, "M-1", True, False, 0),       # NT 13, add stops one row short
    (16391, 200, 216, "1", False, True, 0),         # second block of 8 columns at n0 = 208 (NT 4); no bias; one add row
    (16391, 36, 1000, "M-1", True, True, 0),        # five column blocks, k tail of 4
    (16391, 30, 210, "M", True, True, 0),           # V4 = false, scalar epilogue, second block of 2 columns
    (16391, 30, 72, None, False, False, 0),         # V4 = false, NT 8
    (16391, 32, 8, "M", True, False, 0),            # one k tile, 8 columns
    (16391, 4, 136, "1", True, True, 0),            # K = 4: a single quarter-filled k tile
    (16391, 32, 64, "M", True, True, MIS_A),        # unaligned A: scalar loaders, float4 epilogue
    (16391, 36, 128, None, True, False, MIS_W),     # unaligned W
    (16391, 32, 208, "M-1", True, True, MIS_C),     # unaligned C: float4 loaders, scalar epilogue
    (16391, 4, 72, "M", True, False, MIS_ADD),      # unaligned add: scalar epilogue
    # (MT, NW) = (1, 8)
    (32775, 200, 136, "M-1", True, True, 0),        # NT 13
    (32775, 200, 64, None, True, False, 0),         # NT 4
    (32775, 36, 128, "1", False, False, 0),         # NT 8
    (32775, 30, 1000, "M", True, True, 0),          # V4 = false through five blocks
    (32775, 30, 8, "M-1", True, True, 0),           # V4 = false, NT 4
    (32775, 30, 72, None, True, True, 0),           # V4 = false, NT 8
    (32775, 32, 216, "M-1", True, False, 0),        # n0 = 208
    (32775, 4, 210, "M", True, True, 0),            # scalar epilogue
    (32775, 32, 136, "M", True, True, MIS_A | MIS_C),
    # (MT, NW) = (2, 4)
    (130951, 36, 208, "M-1", True, True, 0),        # NT 13
    (130951, 32, 64, None, True, False, 0),         # NT 4
    (130951, 36, 128, "M", False, True, 0),         # NT 8
    (130951, 4, 1000, "1", True, True, 0),          # five blocks
    (130951, 30, 136, "M-1", True, False, 0),       # V4 = false, NT 13
    (130951, 30, 8, "M", True, True, 0),            # V4 = false, NT 4
    (130951, 30, 72, None, True, False, 0),         # V4 = false, NT 8
    (130951, 32, 216, "M", True, True, 0),          # n0 = 208
    (130951, 4, 210, "M-1", True, False, 0),        # scalar epilogue
    (130951, 4, 72, "M", True, True, MIS_W | MIS_ADD),
]

# gnnrag_linear_pair above the skinny bound: two gnnrag_linear calls (no relu)
_PAIR = [
    (16391, 200, 72, "M-1", True, False, 0),
    (32775, 36, 210, None, True, False, 0),
    (32775, 32, 216, "M", False, False, MIS_C),
]

# ---- gnnrag_update_score (unfused: k-tiled at any M): (BN, D, I, mis), each in all three math modes ------------------
_UPDATE = [
    (71, 30, 1, 0), (71, 56, 2, 0), (71, 100, 1, 0), (71, 128, 2, 0), (71, 200, 1, 0), (71, 208, 2, 0),
    (71, 200, 1, MIS_C), (71, 128, 1, MIS_A1), (71, 208, 1, MIS_W),
    (16391, 56, 2, 0), (16391, 30, 2, 0), (16391, 100, 2, 0), (16391, 128, 1, MIS_A1), (16391, 208, 1, 0),
    (16391, 200, 1, MIS_A), (16391, 56, 1, MIS_C),
    (32775, 56, 1, 0), (32775, 30, 1, 0), (32775, 100, 1, 0), (32775, 128, 1, MIS_A), (32775, 200, 1, 0),
    (32775, 200, 1, MIS_A1),
    (130951, 56, 1, 0), (130951, 30, 1, 0), (130951, 100, 1, 0), (130951, 128, 1, MIS_W), (130951, 200, 1, 0),
    (130951, 200, 1, MIS_A),
]

# ---- gnnrag_update_score_fused: (BN, D, I, math, mis, family) --------------------------------------------------------
# k-tiled (EPI_UPDATE with `add`) where no W-resident / one-wave kernel takes the call: >= 4096 rows in bf16x3 at a
# hidden size the bf16x3 W-resident kernel does not serve, or unaligned operands; the other families for the record.
_FUSED = [
    (16391, 56, 1, 1, 0, KTILED), (16391, 100, 2, 1, 0, KTILED), (32775, 128, 1, 1, 0, KTILED),
    (16391, 200, 1, 0, MIS_ADD, KTILED), (32775, 200, 2, 2, MIS_C, KTILED), (16391, 30, 1, 2, 0, KTILED),
    (130951, 100, 1, 1, 0, KTILED),
    (4095, 200, 1, 0, 0, UPDATE_SKINNY), (4095, 56, 2, 1, 0, UPDATE_SKINNY),
    (4096, 200, 1, 0, 0, WRES), (4096, 100, 1, 2, 0, WRES),
    (8191, 208, 1, 2, 0, KTILED),      # D = 208: the fp32 weight block exceeds a CU's LDS, and below 8192 rows no k_update_b3
    (8192, 200, 1, 1, 0, UPDATE_B3), (8199, 208, 2, 2, 0, UPDATE_B3),
]


def _build():
    cases = []
    for (M, K, Nout, add, bias, relu, mis) in _LINEAR:
        for math in MATHS:
            cases.append(Case("linear", M, K, Nout, math, add, bias, relu, mis, KTILED,
                              _linear_forms(M, K, Nout, math, add, mis)))
    for (M, K, Nout, add, bias, relu, mis) in _PAIR:
        for math in MATHS:
            cases.append(Case("linear_pair", M, K, Nout, math, add, bias, relu, mis, KTILED,
                              _linear_forms(M, K, Nout, math, add, mis)))
    for (BN, D, I, mis) in _UPDATE:
        for math in MATHS:
            cases.append(Case("update_score", BN, D, I, math, None, True, True, mis, KTILED,
                              _update_forms(BN, D, I, math, mis, False)))
    for (BN, D, I, math, mis, family) in _FUSED:
        forms = _update_forms(BN, D, I, math, mis, True) if family == KTILED else ()
        cases.append(Case("update_score_fused", BN, D, I, math, "M", True, True, mis, family, forms))
    return cases


CASES = _build()

# The rounding-class check (random data of wide dynamic range) runs on one case per k-tiled form and K, the first the
# table holds; the exact-arithmetic check runs on every case.
def rounding_cases():
    seen, out = set(), []
    for c in CASES:
        if c.family != KTILED or c.entry == "linear_pair":
            continue
        for f in c.forms:
            key = (f.epi, f.nt, f.mt, f.nw, f.v4, f.math, c.K if f.epi == EPI_LINEAR else (2 * c.N + 1) * c.K)
            if key not in seen:
                seen.add(key)
                if c not in out:
                    out.append(c)
    return out
