"""The split-K linear on the MI355X (csrc/linear_splitk.hip through ``ops.linear_splitk``): exact integer cases, general floats
against float64 within ``bert_oracle.bound`` (4 x the error of the same statement in fp32 torch on the CPU, at least 1e-6,
relative to the oracle's largest entry - never taken from the code under test), and the value rule: a row's bits depend on
its own data, K and the effective (splits, k_chunk) only.  Every figure is printed before it is asserted.

Shapes: M in {1, 16, 17, 37} (one 16-row tile, a full one, two, a group of four with a short last tile) and 70 (two
workgroups of rows); K in {4, 36, 100, 384} (one float4, a chunk shorter than a k step, a short last chunk, several steps);
Nout in {4, 60, 64, 68, 200} (a short column tile, a full one, one column tile and a bit, several); the real FFN-out shape
(12, 3072, 768); splits in {0, 1, 2, 3, the largest legal}.  Not the cross product: each dimension's edges."""
import numpy as np
import pytest
import torch

import bert_oracle as bo

pytestmark = pytest.mark.gpu
MAX = "largest"
EPIS = ("bias", "gelu", "add_ln")
EPS = 1e-12

# (M, K, Nout, splits)
CASES = [(1, 4, 4, 0), (1, 4, 4, MAX), (16, 36, 60, 2), (17, 100, 68, 3), (37, 384, 200, 0), (37, 384, 200, MAX),
         (16, 100, 64, MAX), (17, 36, 200, MAX), (1, 384, 60, 1), (37, 100, 4, 2), (37, 36, 64, 3), (17, 384, 68, 0),
         (70, 100, 68, 3), (12, 3072, 768, 0), (12, 3072, 768, MAX), (12, 3072, 768, 1)]
IDS = ["%dx%dx%d-s%s" % c for c in CASES]


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _splits(M, K, Nout, splits):
    """The forced value a case means (MAX: the largest legal one) and the effective splits the plan must report."""
    from gnnrag_amd import _lib, ops
    if splits == MAX:
        splits = min(K // 4, _lib.SPLITK_MAX_SPLITS)
    plan = ops.linear_splitk_plan(M, K, Nout, splits)
    return splits, plan


_data = {}


def _case(M, K, Nout, integers=False):
    """Seeded operands on the CPU (shared): A, add ~ N(0, 1), W x 0.05, vectors x 0.1, the LayerNorm weight 1 + that (as
    tests/bert_oracle.py scales a model); ``integers``: everything a small integer in [-2, 2]."""
    key = (M, K, Nout, integers)
    if key not in _data:
        rs = np.random.RandomState(1000 * M + 10 * K + Nout)
        if integers:
            d = {n: rs.randint(-2, 3, shp).astype(np.float32)
                 for n, shp in (("A", (M, K)), ("W", (Nout, K)), ("bias", (Nout,)), ("add", (M, Nout)))}
            d["g"], d["b"] = np.ones(Nout, np.float32), np.zeros(Nout, np.float32)
        else:
            d = {"A": rs.standard_normal((M, K)), "W": rs.standard_normal((Nout, K)) * 0.05,
                 "bias": rs.standard_normal(Nout) * 0.1, "add": rs.standard_normal((M, Nout)),
                 "g": 1.0 + rs.standard_normal(Nout) * 0.1, "b": rs.standard_normal(Nout) * 0.1}
        _data[key] = {n: torch.from_numpy(np.asarray(v, dtype=np.float32)) for n, v in d.items()}
    return _data[key]


def _statement(d, epi, dtype):
    """The same statement in torch on the CPU in ``dtype`` (float64: the oracle; float32: the yardstick e_ref)."""
    t = {n: v.to(dtype) for n, v in d.items()}
    x = t["A"] @ t["W"].t() + t["bias"]
    if epi == "gelu":
        return torch.nn.functional.gelu(x)                               # erf
    if epi == "add_ln":
        return torch.nn.functional.layer_norm(x + t["add"], (x.shape[1],), t["g"], t["b"], EPS)
    return x


def _run(dev, d, epi, splits, out=None, add=None, rows=None, cols=None):
    from gnnrag_amd import ops
    sel = (lambda t: t) if rows is None else (lambda t: t[rows].contiguous())
    A, W, bias = sel(d["A"]).to(dev), d["W"].to(dev), d["bias"].to(dev)
    g, b = d["g"].to(dev), d["b"].to(dev)
    if cols is not None:
        W, bias, g, b = W[:cols].contiguous(), bias[:cols].contiguous(), g[:cols].contiguous(), b[:cols].contiguous()
    kw = {}
    if epi == "add_ln":
        if add is None:
            add = sel(d["add"]).to(dev)
            add = add if cols is None else add[:, :cols].contiguous()
        kw = dict(add=add, ln=(g, b, EPS))
    return ops.linear_splitk(A, W, bias, epi=epi, splits=splits, out=out, **kw)


# -- exact ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,K,Nout,splits", CASES, ids=IDS)
def test_small_integers_are_exact(dev, M, K, Nout, splits):
    """Entries in [-2, 2]: every partial sum is an integer below 2^24, so whatever the chunks are the result of BIAS is the
    float64 product bit for bit - a dropped, doubled or misplaced k, row, column or chunk shows as a whole number."""
    forced, plan = _splits(M, K, Nout, splits)
    d = _case(M, K, Nout, integers=True)
    want = _statement(d, "bias", torch.float64)
    assert float(want.abs().max()) < 2 ** 24
    got = _run(dev, d, "bias", forced).cpu()
    wrong = int((got.double() != want).sum())
    print("exact %dx%dx%d splits %s -> plan %s: %d of %d entries differ" % (M, K, Nout, splits, tuple(plan), wrong,
                                                                           want.numel()))
    assert forced == 0 or plan.splits == forced
    assert got.shape == (M, Nout) and wrong == 0


def test_no_bias_is_exact(dev):
    from gnnrag_amd import ops
    d = _case(17, 100, 68, integers=True)
    got = ops.linear_splitk(d["A"].to(dev), d["W"].to(dev), None, splits=3).cpu()
    assert torch.equal(got.double(), d["A"].double() @ d["W"].double().t())


# -- general floats -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("M,K,Nout,splits", CASES, ids=IDS)
def test_floats_against_float64(dev, M, K, Nout, splits, epi):
    forced, plan = _splits(M, K, Nout, splits)
    d = _case(M, K, Nout)
    want = _statement(d, epi, torch.float64).numpy()
    e_ref = bo.rel_err(_statement(d, epi, torch.float32).numpy(), want)
    got = _run(dev, d, epi, forced)
    err = bo.rel_err(got.cpu().numpy(), want)
    print("%s %dx%dx%d splits %s -> plan %s: err %.3g, e_ref %.3g, bound %.3g"
          % (epi, M, K, Nout, splits, tuple(plan), err, e_ref, bo.bound(e_ref)))
    # form: the plan reports the splits this case means to exercise (a moved rule must not empty a case)
    if forced:
        assert plan.splits == forced and plan.k_chunk == -(-(-(-K // forced)) // 4) * 4
    else:
        assert plan.splits >= 2 if K >= 100 else plan.splits == 1
    assert plan.launches == 2 and plan.splits * plan.k_chunk >= K > (plan.splits - 1) * plan.k_chunk
    assert got.shape == (M, Nout)
    assert err <= bo.bound(e_ref)
    assert torch.equal(got, _run(dev, d, epi, forced))                  # two identical calls: equal bits


# every width at which the LayerNorm reduce takes another kernel: 1, 2, 4, 8, 16 float4 per lane, and rows past the registers
@pytest.mark.parametrize("Nout", [256, 260, 512, 516, 1028, 2052, 4096, 4100])
def test_layernorm_row_widths(dev, Nout):
    M, K = 3, 36
    d = _case(M, K, Nout)
    want = _statement(d, "add_ln", torch.float64).numpy()
    e_ref = bo.rel_err(_statement(d, "add_ln", torch.float32).numpy(), want)
    got = _run(dev, d, "add_ln", 2)
    err = bo.rel_err(got.cpu().numpy(), want)
    print("add_ln Nout=%d: err %.3g, e_ref %.3g, bound %.3g" % (Nout, err, e_ref, bo.bound(e_ref)))
    assert err <= bo.bound(e_ref)
    add = d["add"].to(dev).clone()
    assert _run(dev, d, "add_ln", 2, out=add, add=add) is add and torch.equal(add, got)      # C aliasing add


# -- the value rule -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("K,Nout,splits", [(384, 200, 0), (384, 200, 3), (100, 68, MAX), (36, 60, 2)])
def test_a_row_does_not_depend_on_the_rows_around_it(dev, K, Nout, splits, epi):
    """Row r of the M = 37 call (a group of four row tiles) against the M = 1 call on that row (one tile), and the first 17
    rows against the M = 17 call (two tiles): equal bits at equal forced splits and at splits = 0."""
    forced, plan = _splits(37, K, Nout, splits)
    assert _splits(1, K, Nout, splits)[1] == plan == _splits(17, K, Nout, splits)[1]
    d = _case(37, K, Nout)
    full = _run(dev, d, epi, forced)
    for r in (0, 15, 16, 36):
        assert torch.equal(_run(dev, d, epi, forced, rows=slice(r, r + 1)), full[r:r + 1]), r
    assert torch.equal(_run(dev, d, epi, forced, rows=slice(0, 17)), full[:17])


@pytest.mark.parametrize("epi", ["bias", "gelu"])
@pytest.mark.parametrize("splits", [1, 3, MAX])
def test_a_column_does_not_depend_on_the_columns_around_it(dev, splits, epi):
    """The Nout = 64 call on W[:64] against the first 64 columns of the Nout = 200 call, at equal forced splits."""
    forced, plan = _splits(37, 384, 200, splits)
    assert _splits(37, 384, 64, splits)[1] == plan and plan.splits == forced
    d = _case(37, 384, 200)
    full = _run(dev, d, epi, forced)
    part = _run(dev, d, epi, forced, cols=64)
    assert part.shape == (37, 64) and torch.equal(part, full[:, :64])


@pytest.mark.parametrize("M,K,Nout,splits", [(17, 100, 68, 3), (37, 384, 200, 0), (12, 3072, 768, 0)])
def test_layernorm_into_the_buffer_of_add(dev, M, K, Nout, splits):
    d = _case(M, K, Nout)
    fresh = _run(dev, d, "add_ln", splits)
    add = d["add"].to(dev).clone()
    out = _run(dev, d, "add_ln", splits, out=add, add=add)
    assert out is add and torch.equal(out, fresh)
