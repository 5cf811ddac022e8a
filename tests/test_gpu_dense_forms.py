"""The dense kernels form by form (tests/dense_cases.py; tests/test_dense_forms_host.py proves that table's coverage on
the host): every case first asserts with ``ops.dense_form`` that the call runs the kernel form it is there for, then
checks values against float64.

* Exact arithmetic.  All operands are integer-valued floats in [-3, 3]: every partial sum is an integer far below
  2**24 and a small integer lies entirely in the high bf16 plane, so the fp32 MFMA chain AND the bf16x3 form must equal
  the float64 product bit for bit - a wrong k position, a dropped k tail, a wrong column block or `add` row has no
  tolerance to hide behind.  The reference's own exactness is asserted on the host (``want == float32(want)``, bound
  of the partial sums below 2**24).  Masked rows carry zero inputs (|score| < 4096, half an ulp of 1e11), so their
  score is exactly -1e11.
* Rounding class.  Data of test_bf16x3_linear_is_fp32_class (rows scaled by exp(U(-6, 6)), W / sqrt(K)); metric
  e = max |got - want64| / S with S = |A||W|^T + |b| (+ |add|); yardstick e_cpu32, the same quantity for numpy's float32
  product on the CPU: e <= 8 * max(e_cpu32, 6e-8), and the absolute cap e <= 4e-7, both over every entry of the
  output (the reference is formed 16384 rows at a time).  Two calls are bit-identical.  GNNRAG_DENSE_FORMS_TABLE=<file>
  appends the measured (form, K, math, e, e_cpu32) lines to a file (profiles/dense_forms_rounding.txt was recorded that
  way).
"""
import functools
import os

import numpy as np
import pytest
import torch

import dense_cases as dc

pytestmark = pytest.mark.gpu

E_CAP = 4e-7          # the project's absolute cap on e (test_bf16x3_linear_is_fp32_class)
E_FACTOR, E_FLOOR = 8, 6e-8


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _assert_form(c):
    """The case runs the kernel form it names (same assertion as tests/test_dense_forms_host.py)."""
    from gnnrag_amd import ops
    q = lambda blk: ops.dense_form(c.entry, c.M, c.K, c.N, math=c.math, add_rows=dc.add_rows(c), misaligned=c.mis,
                                   block=blk)
    f = q(0)
    assert f.family == c.family == f.block_family, (f, c)
    for blk, want in enumerate(c.forms):
        f = q(blk)
        assert dc.KForm(f.epi, f.nt, f.mt, f.nw, f.v4, f.math, f.v4out, f.n0) == want, (blk, c)


def _put(dev, a, misaligned):
    """Host array -> device tensor; ``misaligned``: a contiguous view one float into a larger buffer (4 bytes past a
    16-byte boundary)."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not misaligned:
        d = t.to(dev)
        assert d.data_ptr() % 16 == 0
        return d
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    d = buf[1:].view(t.shape)
    d.copy_(t)
    assert d.data_ptr() % 16 == 4 and d.is_contiguous()
    return d


def _out(dev, shape, misaligned):
    n = int(np.prod(shape))
    buf = torch.empty(n + 1, dtype=torch.float32, device=dev)
    return buf[1:].view(shape) if misaligned else buf[:n].view(shape)


def _p(t):
    return None if t is None else t.data_ptr()


def _run(dev, c, d):
    """One call of the case's entry point on the host arrays ``d``; returns the outputs as device tensors.  Aligned
    linear / update calls go through the ops wrappers, everything else through the C ABI directly."""
    from gnnrag_amd import _lib, ops
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    mis = c.mis
    if c.entry in ("linear", "linear_pair"):
        A = _put(dev, d["A"], mis & dc.MIS_A)
        W = _put(dev, d["W"], mis & dc.MIS_W)
        b = _put(dev, d["b"], 0)
        add = _put(dev, d["add"], mis & dc.MIS_ADD)
        ar = 0 if add is None else add.shape[0]
        if c.entry == "linear":
            if not mis:
                return (ops.linear(A, W, b, add, relu=c.relu, math=c.math),)
            C = _out(dev, (c.M, c.N), mis & dc.MIS_C)
            _lib.check(lib.gnnrag_linear(A.data_ptr(), c.M, c.K, W.data_ptr(), _p(b), _p(add), ar, int(c.relu),
                                         C.data_ptr(), c.N, c.math, st), "gnnrag_linear")
            return (C,)
        A1 = _put(dev, d["A1"], mis & dc.MIS_A)
        add1 = _put(dev, d["add1"], mis & dc.MIS_ADD)
        C0, C1 = _out(dev, (c.M, c.N), mis & dc.MIS_C), _out(dev, (c.M, c.N), mis & dc.MIS_C)
        _lib.check(lib.gnnrag_linear_pair(A.data_ptr(), A1.data_ptr(), c.M, c.K, W.data_ptr(), _p(b), _p(add), _p(add1),
                                          ar, C0.data_ptr(), C1.data_ptr(), c.N, c.math, st), "gnnrag_linear_pair")
        return (C0, C1)
    BN, D, I = c.M, c.K, c.N
    h = _put(dev, d["h"], mis & dc.MIS_A)
    W = _put(dev, d["W"], mis & dc.MIS_W)
    b, w_s, b_s, mask = (_put(dev, d[k], 0) for k in ("b", "w_s", "b_s", "mask"))
    if c.entry == "update_score":
        x = _put(dev, d["agg"], mis & dc.MIS_A1)
        if not mis:
            return ops.update_score(h, x, W, b, w_s, b_s, mask, I, math=c.math)
        fn, name = lib.gnnrag_update_score, "gnnrag_update_score"
    else:
        x = _put(dev, d["nbr"], mis & dc.MIS_ADD)
        if not mis:
            return ops.update_score_fused(h, x, W, b, w_s, b_s, mask, I, math=c.math)
        fn, name = lib.gnnrag_update_score_fused, "gnnrag_update_score_fused"
    h_out = _out(dev, (BN, D), mis & dc.MIS_C)
    score = torch.empty(BN, dtype=torch.float32, device=dev)
    _lib.check(fn(h.data_ptr(), x.data_ptr(), W.data_ptr(), b.data_ptr(), w_s.data_ptr(), b_s.data_ptr(),
                  mask.data_ptr(), h_out.data_ptr(), score.data_ptr(), BN, D, I, c.math, st), name)
    return h_out, score


def _mask(rng, BN):
    m = (rng.random(BN) < 0.75).astype(np.float32)
    m[-1] = 0.0                      # the ragged last tile holds a masked row ...
    m[-2] = 1.0                      # ... next to a live one
    return m


# ---- exact arithmetic ------------------------------------------------------------------------------------------------

def _ints(rng, *shape):
    return rng.integers(-3, 4, size=shape).astype(np.float32)


@functools.lru_cache(maxsize=1)
def _exact_data(kind, M, K, N, add, bias, relu):
    """Inputs and the float64 result of one problem, shared by the cases that differ in math mode / alignment only."""
    rng = np.random.default_rng([M, K, N, len(kind)])
    if kind in ("linear", "linear_pair"):
        ar = {None: 0, "M": M, "M-1": M - 1, "1": 1}[add]
        d = {"A": _ints(rng, M, K), "W": _ints(rng, N, K), "b": _ints(rng, N) if bias else None,
             "add": _ints(rng, ar, N) if ar else None, "A1": None, "add1": None}
        if kind == "linear_pair":
            d["A1"] = _ints(rng, M, K)
            d["add1"] = _ints(rng, ar, N) if ar else None
        bound = 9 * K + 3 + 3
        want = []
        for A, ad in ((d["A"], d["add"]),) + (((d["A1"], d["add1"]),) if kind == "linear_pair" else ()):
            w = A.astype(np.float64) @ d["W"].astype(np.float64).T
            if bias:
                w += d["b"]
            if ad is not None:
                w[:ar] += ad
            want.append(np.maximum(w, 0) if relu else w)
    else:
        BN, D, I = M, K, N
        Kc = (2 * I + 1) * D
        mask = _mask(rng, BN)
        live = mask[:, None]
        d = {"h": _ints(rng, BN, D) * live, "W": _ints(rng, D, Kc), "b": _ints(rng, D), "w_s": _ints(rng, D),
             "b_s": _ints(rng, 1), "mask": mask}
        W64 = d["W"].astype(np.float64)
        if kind == "update_score":
            d["agg"] = _ints(rng, BN, 2 * I * D) * live
            pre = np.concatenate([d["h"], d["agg"]], 1).astype(np.float64) @ W64.T + d["b"]
            bound = 9 * Kc + 3
        else:
            d["nbr"] = _ints(rng, BN, D) * live
            pre = d["h"].astype(np.float64) @ W64[:, :D].T + d["b"] + d["nbr"]
            bound = 9 * D + 3 + 3
        hn = np.maximum(pre, 0)
        s = hn @ d["w_s"].astype(np.float64) + d["b_s"][0]
        bound = max(bound, 3 * D * hn.max() + 3)
        assert np.abs(s[mask == 0]).max() < 4096          # half an ulp of 1e11: the masked sum rounds to -1e11 exactly
        want = [hn, np.where(mask != 0, s, np.float64(np.float32(-1e11)))]
    # the reference itself is exact in fp32: integer partial sums below 2**24
    assert bound < 2 ** 24
    for w in want:
        assert np.array_equal(w, w.astype(np.float32).astype(np.float64))
    return d, [w.astype(np.float32) for w in want]


@pytest.mark.parametrize("c", dc.CASES, ids=dc.case_id)
def test_exact_integer_arithmetic(dev, c):
    """Integer-valued operands: C / h' / the live scores equal the float64 result bit for bit in every math mode,
    masked scores are exactly -1e11."""
    _assert_form(c)
    d, want = _exact_data(c.entry, c.M, c.K, c.N, c.add, c.bias, c.relu)
    got = [t.cpu().numpy() for t in _run(dev, c, d)]
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        g = g.reshape(w.shape)
        bad = np.flatnonzero((g != w).ravel())
        assert bad.size == 0, "output %d: %d differing entries, first at %s: got %r want %r" % (
            j, bad.size, np.unravel_index(bad[0], w.shape), g.ravel()[bad[0]], w.ravel()[bad[0]])
    if c.entry.startswith("update"):
        assert (got[1][d["mask"] == 0] == np.float32(-1e11)).all()


# ---- rounding class --------------------------------------------------------------------------------------------------

CHUNK = 16384        # rows per float64 product: bounds the host memory of the reference, every row is covered


def _rounding_inputs(c):
    """Random inputs of wide dynamic range (test_bf16x3_linear_is_fp32_class: rows scaled by exp(U(-6, 6)), W/sqrt(K))."""
    M, K, N = c.M, c.K, c.N
    rng = np.random.default_rng([M, K, N, 7])
    scale = np.exp(rng.uniform(-6, 6, (M, 1)))
    f32 = np.float32
    if c.entry == "linear":
        ar = dc.add_rows(c) or 0
        return {"A": (rng.standard_normal((M, K)) * scale).astype(f32),
                "W": (rng.standard_normal((N, K)) / np.sqrt(K)).astype(f32),
                "b": rng.standard_normal(N).astype(f32) if c.bias else None,
                "add": (rng.standard_normal((ar, N)) * scale[:ar]).astype(f32) if ar else None}
    BN, D, I = M, K, N
    Kc = (2 * I + 1) * D
    d = {"h": (rng.standard_normal((BN, D)) * scale).astype(f32),
         "W": (rng.standard_normal((D, Kc)) / np.sqrt(Kc)).astype(f32), "b": rng.standard_normal(D).astype(f32),
         "w_s": (rng.standard_normal(D) / np.sqrt(D)).astype(f32), "b_s": rng.standard_normal(1).astype(f32),
         "mask": _mask(rng, BN)}
    if c.entry == "update_score":
        d["agg"] = (rng.standard_normal((BN, 2 * I * D)) * scale).astype(f32)
    else:
        d["nbr"] = (rng.standard_normal((BN, D)) * scale).astype(f32)
    return d


def _emax(got, want64, S):
    return float((np.abs(got.astype(np.float64) - want64) / S).max()) if want64.size else 0.0


def _rounding_errors(c, d, got):
    """e = max |got - want64| / S and e_cpu32 (the same for numpy's float32 chain) over EVERY row, per output: the
    float64 product, S and the float32 product are formed CHUNK rows at a time.  Returns [(name, e, e_cpu32)]."""
    f64 = np.float64
    e = {"out": [0.0, 0.0], "score": [0.0, 0.0]}
    upd = c.entry != "linear"
    W = d["W"] if c.entry != "update_score_fused" else np.ascontiguousarray(d["W"][:, :c.K])
    W64, Wabs = W.astype(f64), np.abs(W).astype(f64)
    ar = 0 if upd else (dc.add_rows(c) or 0)
    for r0 in range(0, c.M, CHUNK):
        r1 = min(c.M, r0 + CHUNK)
        if c.entry == "linear":
            A, bias, add = d["A"][r0:r1], d["b"], (d["add"][r0:min(r1, ar)] if ar > r0 else None)
        elif c.entry == "update_score":
            A, bias, add = np.concatenate([d["h"][r0:r1], d["agg"][r0:r1]], 1), d["b"], None
        else:
            A, bias, add = d["h"][r0:r1], d["b"], d["nbr"][r0:r1]
        want = A.astype(f64) @ W64.T
        S = np.abs(A).astype(f64) @ Wabs.T
        cpu = A @ W.T
        if bias is not None:
            want += bias; S += np.abs(bias); cpu = cpu + bias
        if add is not None:
            n = add.shape[0]
            want[:n] += add; S[:n] += np.abs(add); cpu[:n] = cpu[:n] + add
        if upd or c.relu:                    # relu is 1-Lipschitz: the bound e * S carries over
            want, cpu = np.maximum(want, 0), np.maximum(cpu, 0)
        e["out"][0] = max(e["out"][0], _emax(got[0][r0:r1], want, S))
        e["out"][1] = max(e["out"][1], _emax(cpu, want, S))
        if upd:
            ws = d["w_s"]
            live = d["mask"][r0:r1] != 0
            s = want @ ws.astype(f64) + d["b_s"][0]
            # the score inherits the h' errors (<= e * S per entry) through |w_s| and adds its own dot product's rounding
            Ss = (S + np.abs(want)) @ np.abs(ws).astype(f64) + np.abs(d["b_s"][0])
            sc = cpu @ ws + d["b_s"][0]
            e["score"][0] = max(e["score"][0], _emax(got[1][r0:r1][live], s[live], Ss[live]))
            e["score"][1] = max(e["score"][1], _emax(sc[live], s[live], Ss[live]))
    return [(k, v[0], v[1]) for k, v in e.items() if upd or k == "out"]


# (epi, nt, mt, nw, v4, math, K) forms that exceed the absolute cap while meeting the 8x rule, which then governs them
# alone (profiles/dense_forms_rounding.txt)
CAP_EXEMPT = frozenset()


@pytest.mark.parametrize("c", dc.rounding_cases(), ids=dc.case_id)
def test_rounding_class(dev, c):
    """fp32-class error per k-tiled form and K, against numpy's float32 product as the yardstick; bit-reproducible."""
    _assert_form(c)
    d = _rounding_inputs(c)
    out = _run(dev, c, d)
    again = _run(dev, c, d)
    for a, b in zip(out, again):
        assert torch.equal(a, b), "two calls on the same inputs differ"
    got = [t.cpu().numpy() for t in out]
    if len(got) == 2:
        assert (got[1][d["mask"] == 0] <= -9.9e10).all()
    f = c.forms[0]
    Kk = c.K if f.epi == dc.EPI_LINEAR else (c.K if c.entry == "update_score_fused" else (2 * c.N + 1) * c.K)
    line = _rounding_errors(c, d, got)
    forms = sorted({(x.epi, x.nt, x.mt, x.nw, x.v4, x.math) for x in c.forms})
    text = "%-18s M=%-6d K=%-4d N=%-4d math=%d forms(epi,nt,mt,nw,v4,math)=%s  %s" % (
        c.entry, c.M, Kk, c.N, c.math, forms, "  ".join("%s: e=%.3g e_cpu32=%.3g" % t for t in line))
    print(text)
    if os.environ.get("GNNRAG_DENSE_FORMS_TABLE"):
        with open(os.environ["GNNRAG_DENSE_FORMS_TABLE"], "a") as fh:
            fh.write(text + "\n")
    for name, e, e_cpu in line:
        assert e <= E_FACTOR * max(e_cpu, E_FLOOR), (name, e, e_cpu)
        if not any((x.epi, x.nt, x.mt, x.nw, x.v4, x.math, Kk) in CAP_EXEMPT for x in c.forms):
            assert e <= E_CAP, (name, e, e_cpu)
