"""The launches in front of a seed layer, held to the bits of the library before the relation projections' loads were
rescheduled and the frontier build moved into their launch (tests/golden/seed_prologue_parent.json):

* the combined launch (gnnrag_seed_prologue) against the two stand-alone calls it stands for, byte for byte: T, the
  packed operand, every question's counts, lists, flags, seeds, the zeroed score and zero row, guard bytes behind each.
* k_rel_transform alone - T, the public bf16 planes and the packed operand, both tile counts per wave (R1 <= 2048 and
  above), with and without position rows.  test_gpu_tables_packed / test_gpu_b3_planes hold the same values to numpy;
  this holds them to what the library wrote before.
* whole layer stacks that start from a seed distribution (GNNRAG_PATH_SEED_PRIOR, bf16x3): every layer's dist and the
  final h, for the W-resident update with row gates + the V-form tables, the same with position rows, and the
  small-batch kernels; a second run on the projections the first left in the workspace; a captured and replayed sequence.
* k_softmax_pairs against the two launches it stands for (GNNRAG_SOFTMAX_PAIRS=0: k_masked_softmax, then the walk's
  own pass over the facts), through everything the later layers compute from the pairs.

The digests were recorded with the library of the commit before this module existed (`record()` below, run once with
GNNRAG_LIB pointing at that build); they are never regenerated from the code under test.
"""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from test_gpu_tables_sparse import _plan

pytestmark = pytest.mark.gpu

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seed_prologue_parent.json")


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=1)
def _golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(dev)


def digest(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


# ---- the combined launch against the two stand-alone calls -----------------------------------------------------------------

KINDS = ("one", "three", "none", "forty", "all")      # seeds of a question; "forty" > the 32 the walk lists, "all": every
#                                                       node, at N = 2100 more than the 2048 the build keeps (all flagged)
#             R1    D    L  pos    B  N     kind of question 0 (B = 5: one question of every kind)
PROLOGUE = [(1,    200, 1, False, 1, 48,   "one"),
            (63,   208, 3, True,  5, 48,   None),
            (64,   56,  8, False, 5, 2100, None),
            (65,   200, 3, True,  5, 2100, None),
            (601,  208, 8, False, 1, 2100, "all"),
            (601,  200, 3, True,  5, 2100, None),
            (601,  56,  1, True,  5, 48,   None),
            (2049, 200, 3, True,  5, 48,   None),        # more rows than the one launch takes: the two launches
            (65,   56,  9, True,  1, 48,   "forty"),     # more layers than one launch takes: the two launches
            (65,   208, 1, False, 1, 2100, "none"),
            (64,   200, 3, False, 1, 48,   "three")]


def _prologue_dist(rng, B, N, first):
    d = np.zeros((B, N), dtype=f32)
    for b in range(B):
        kind = first if B == 1 else KINDS[b]
        k = {"one": 1, "three": 3, "none": 0, "forty": 40, "all": N}[kind]
        if k:
            d[b, rng.choice(N, size=k, replace=False)] = 1.0 / k
    return d


@pytest.mark.parametrize("R1,D,L,pos,B,N,first", PROLOGUE)
def test_seed_prologue_equals_the_stand_alone_calls(dev, R1, D, L, pos, B, N, first):
    from gnnrag_amd import _lib, ops
    lib = _lib.load()
    rng = np.random.default_rng([R1, D, L, B, N])
    F = 6 * N
    h = np.concatenate([b * N + rng.integers(0, N, F) for b in range(B)]).astype(np.int64)
    t = np.concatenate([b * N + rng.integers(0, N, F) for b in range(B)]).astype(np.int64)
    r = rng.integers(0, R1, B * F).astype(np.int64)
    plan = ops.CsrPlan(h, r, t, B, N, R1, dev)
    rel = [_t(dev, rng.standard_normal((R1, D))) for _ in range(2)]
    layers = []
    for _ in range(L):
        pe = [_t(dev, 0.5 * rng.standard_normal((R1 - 3, D))) for _ in range(2)] if pos else [None, None]
        layers.append((_t(dev, rng.standard_normal((D, D)) / np.sqrt(D)), _t(dev, 0.1 * rng.standard_normal(D)), pe[0], pe[1]))
    dist = _t(dev, _prologue_dist(rng, B, N, first))
    packed = D != 56
    # the stand-alone calls
    if packed:
        T_want, pk_want = ops.rel_transform(rel[0], rel[1], layers, packed=True)
    else:
        T_want, pk_want = ops.rel_transform(rel[0], rel[1], layers), None
    fr = ops.Frontier(plan, dist)
    # the combined launch into guarded buffers
    GUARD, SENT = 64, 1.2345e30
    nT = L * 2 * R1 * D
    T_buf = torch.full((nT + GUARD,), SENT, device=dev)
    pk_bytes = lib.gnnrag_rel_packed_bytes(R1, D, L) if packed else 0
    pk_buf = torch.full((pk_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev) if packed else None
    lay = ops.frontier_layout(plan)
    assert lay["total"] == lib.gnnrag_frontier_workspace_bytes(plan.c)
    ws = torch.full((lay["total"] + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    score = torch.full((B * N + GUARD,), float("nan"), device=dev)
    zrow = torch.full((D + GUARD,), float("nan"), device=dev)
    combined = ops.seed_prologue(plan, dist, ws, rel[0], rel[1], layers, T_buf, pk_buf, zero_a=score[:B * N], zero_b=zrow[:D])
    torch.cuda.synchronize()
    assert combined == (R1 <= 2048 and L <= 8), "which launch ran"
    assert torch.equal(T_buf[:nT].view(L, 2, R1, D), T_want), "T"
    assert (T_buf[nT:] == SENT).all(), "bytes behind T"
    if packed:
        assert torch.equal(pk_buf[:pk_bytes].view(pk_want.shape), pk_want), "the packed operand"
        assert (pk_buf[pk_bytes:] == 0xA5).all(), "bytes behind the packed operand"
    assert (score[:B * N] == 0).all() and torch.isnan(score[B * N:]).all(), "the score buffer and the bytes behind it"
    assert (zrow[:D] == 0).all() and torch.isnan(zrow[D:]).all(), "the zero row and the bytes behind it"
    assert (ws[lay["total"]:] == 0xA5).all(), "bytes behind the frontier workspace"
    got, want = ws.cpu().numpy(), fr.ws.cpu().numpy()

    def part(buf, name, n, dtype=np.int32):
        return np.frombuffer(buf[lay[name]:lay[name] + n * np.dtype(dtype).itemsize].tobytes(), dtype=dtype)

    rel_off = np.concatenate([[0], np.cumsum(np.bincount(plan.rel_rows()[:, 0], minlength=B))])
    cg, cw = part(got, "counts", 2 * B).reshape(B, 2), part(want, "counts", 2 * B).reshape(B, 2)
    assert np.array_equal(cg, cw), "both counts of every question"
    assert np.array_equal(part(got, "row_flag", B * N + 64, np.uint8), part(want, "row_flag", B * N + 64, np.uint8)), "row gates"
    assert np.array_equal(part(got, "tflag", plan.rel_total, np.uint8), part(want, "tflag", plan.rel_total, np.uint8))
    si_g, si_w = part(got, "seedinfo", 2 * B).reshape(B, 2), part(want, "seedinfo", 2 * B).reshape(B, 2)
    assert np.array_equal(si_g, si_w), "seedinfo"
    rows_g, rows_w = part(got, "rows", B * N), part(want, "rows", B * N)
    tr_g, tr_w = part(got, "trows", plan.rel_total), part(want, "trows", plan.rel_total)
    sd_g, sd_w = part(got, "seeds", 32 * B).reshape(B, 32), part(want, "seeds", 32 * B).reshape(B, 32)
    for b in range(B):
        assert np.array_equal(rows_g[b * N:b * N + cw[b, 0]], rows_w[b * N:b * N + cw[b, 0]]), "node list of question %d" % b
        o = int(rel_off[b])
        assert np.array_equal(tr_g[o:o + cw[b, 1]], tr_w[o:o + cw[b, 1]]), "relation-row list of question %d" % b
        if si_w[b, 0] > 0:
            assert np.array_equal(sd_g[b, :si_w[b, 0]], sd_w[b, :si_w[b, 0]]), "seed list of question %d" % b
    kinds = [first] if B == 1 else list(KINDS)
    for b, kind in enumerate(kinds):                            # the cases are what they say
        nseed = {"one": 1, "three": 3, "none": 0, "forty": 40, "all": N}[kind]
        assert si_w[b, 0] == (nseed if nseed <= 32 else -1)
        if kind == "all" and N > 2048:
            assert cw[b, 0] == N
        if kind == "none":
            assert tuple(cw[b]) == (0, 0)


# ---- k_rel_transform alone ---------------------------------------------------------------------------------------------

RT_CASES = [(R1, D, pos) for R1 in (65, 601, 2049) for D in (200, 208, 56) for pos in (False, True)]


def rt_digests(dev, R1, D, pos, L=3):
    """T [L, 2, R1, D] of the three forms of the call (they must agree), the planes and the packed operand."""
    from gnnrag_amd import ops
    rng = np.random.default_rng([R1, D, int(pos), 11])
    rel = [_t(dev, rng.standard_normal((R1, D))) for _ in range(2)]
    layers = []
    for _ in range(L):
        pe = [_t(dev, 0.5 * rng.standard_normal((R1 - 3, D))) for _ in range(2)] if pos else [None, None]
        layers.append((_t(dev, rng.standard_normal((D, D)) / np.sqrt(D)), _t(dev, 0.1 * rng.standard_normal(D)), pe[0], pe[1]))
    T = ops.rel_transform(rel[0], rel[1], layers)
    T2, planes = ops.rel_transform(rel[0], rel[1], layers, planes=True)
    T3, packed = ops.rel_transform(rel[0], rel[1], layers, packed=True)
    assert torch.equal(T, T2) and torch.equal(T, T3), "T depends on the side output asked for"
    assert torch.isfinite(T).all()
    return {"T": digest(T), "planes": digest(planes), "packed": digest(packed)}


def _rt_key(R1, D, pos):
    return "rt_r%d_d%d_pos%d" % (R1, D, int(pos))


@pytest.mark.parametrize("R1,D,pos", RT_CASES)
def test_rel_transform_bits_of_the_parent(dev, R1, D, pos):
    assert rt_digests(dev, R1, D, pos) == _golden()[_rt_key(R1, D, pos)]


# ---- seed-prior layer stacks -------------------------------------------------------------------------------------------

#              name               B  N     D    I  L  pos    relations
STACKS = {"b5_n1700_d200_i2_l3": (5, 1700, 200, 2, 3, False, 600),
          "b5_n1700_d208_i1_l2_pos": (5, 1700, 208, 1, 2, True, 600),
          "b1_n2000_d56_i2_l3": (1, 2000, 56, 2, 3, False, 1300)}


@functools.lru_cache(maxsize=None)
def _stack(name):
    """The stack of a case and its inputs: one to three seeds per question, each the head of one of its facts."""
    from gnnrag_amd import _lib, ops, synth
    dev = torch.device("cuda", 0)
    B, N, D, I, L, pos, R = STACKS[name]
    if B > 1:
        cfg, plan, _ = _plan(B, R, None, I, N, D)              # (rel_total >= 1024: the V form of the tables)
        assert B * N >= 8192                                    # the gated W-resident bf16x3 update
    else:
        cfg = synth.GraphConfig(name="seedp", B=B, N=N, E=6 * N, R=R, D=D, I=I, L=1, T=1, seed=B + R, n_real_min=N // 3)
        et = synth.make_batch(cfg).edge_tuple
        plan = ops.CsrPlan(et[0], et[1], et[2], cfg.B, cfg.N, cfg.R1, dev)
    R1 = cfg.R1
    rng = np.random.default_rng([B, N, D, I, L])
    relf = [_t(dev, rng.standard_normal((R1, D))) for _ in range(2)]
    layers = []
    for _ in range(L):
        pe = [_t(dev, 0.1 * rng.standard_normal((R1 - 3, D))) for _ in range(2)] if pos else [None, None]
        layers.append((_t(dev, rng.standard_normal((D, D)) / np.sqrt(D) * 0.4), _t(dev, 0.1 * rng.standard_normal(D)),
                       _t(dev, rng.standard_normal((D, (2 * I + 1) * D)) / np.sqrt((2 * I + 1) * D)),
                       _t(dev, 0.1 * rng.standard_normal(D)), pe[0], pe[1]))
    w_s, b_s = _t(dev, rng.standard_normal(D) / np.sqrt(D)), _t(dev, [0.1])
    mask = (rng.random(B * N) < 0.8).astype(f32)
    h0 = _t(dev, 0.5 * rng.standard_normal((B * N, D)))
    d0 = np.zeros((B, N), dtype=f32)
    hd = np.asarray(synth.make_batch(cfg).edge_tuple[0])       # (the batch the plan was built from: heads, global ids)
    for b in range(B):
        own = np.unique(hd[(hd >= b * N) & (hd < (b + 1) * N)])
        k = 1 + b % 3
        pick = rng.choice(own, size=k, replace=False)
        d0[b, pick - b * N] = 1.0 / k
        mask[pick] = 1.0
    ins = _t(dev, 0.3 * rng.standard_normal((B, I, D)))
    st = ops.LayerStack(plan, relf[0], relf[1], layers, w_s, b_s, _t(dev, mask), I,
                        path=_lib.PATH_FUSED | _lib.PATH_SEED_PRIOR, math=ops.MATH_BF16X3)
    return st, h0, _t(dev, d0), ins, L


def stack_digests(out, L):
    h, score, dist = out
    return {"dist": [digest(dist[j]) for j in range(L)], "h_final": digest(h[L - 1])}


@functools.lru_cache(maxsize=None)
def _stack_runs(name):
    """(first run, second run on the projections the first left behind) - computed once, shared, never written to."""
    st, h0, d0, ins, L = _stack(name)
    st.new_forward()
    first = st.run(h0, d0, ins)
    second = st.run(h0, d0, ins)
    torch.cuda.synchronize()
    return first, second


@pytest.mark.parametrize("name", list(STACKS))
def test_seed_stack_bits_of_the_parent(dev, name):
    first, second = _stack_runs(name)
    L = STACKS[name][4]
    assert torch.isfinite(first[0]).all() and torch.isfinite(first[2]).all()
    assert stack_digests(first, L) == _golden()["stack_" + name], "every layer's dist and the final h"
    for a, b in zip(first, second):
        assert torch.equal(a, b), "the run on reused projections differs"


def test_seed_stack_captured_equals_eager(dev):
    name = "b5_n1700_d200_i2_l3"
    first, _ = _stack_runs(name)
    st, h0, d0, ins, L = _stack(name)
    st.capture(h0, d0, ins)
    try:
        got = [x.clone() for x in st.replay(first=True)]
        torch.cuda.synchronize()
    finally:
        st.release_graph()
    for a, b in zip(first, got):
        assert torch.equal(a, b), "the replayed sequence differs from the eager one"


# ---- k_softmax_pairs -----------------------------------------------------------------------------------------------------

def _pairs_plan(N, weights):
    """Three questions: one with facts, one without any, one whose merged record count (2 x its facts) is no multiple of
    parts x 1024 (8 parts at B = 3)."""
    from gnnrag_amd import ops
    B, R1 = 3, 40
    rng = np.random.default_rng([N, 3])
    counts = [10 * N, 0, 7 * N + 333]
    assert (2 * counts[2]) % (8 * 1024) != 0
    h, r, t = [], [], []
    for b, n in enumerate(counts):
        h.append(b * N + rng.integers(0, N, n))
        t.append(b * N + rng.integers(0, N, n))
        r.append(rng.integers(0, R1 - 2, n))
    h, r, t = (np.concatenate(x).astype(np.int64) for x in (h, r, t))
    plan = ops.CsrPlan(h, r, t, B, N, R1, torch.device("cuda", 0))
    if weights:
        outdeg = np.bincount(h, minlength=B * N).astype(np.float64)
        plan.attach_w_gnn((1.0 / outdeg[h]).astype(f32))
    return plan, B, R1


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("N", [48, 2000, 2100])
def test_softmax_pairs_equals_the_two_launches(dev, N, weights, monkeypatch):
    from gnnrag_amd import _lib, ops
    D, I, L = 56, 1, 3
    plan, B, R1 = _pairs_plan(N, weights)
    variant = ops.aggregate_fused_variant(plan, D)
    print("N=%d weights=%d: fused walk variant %d" % (N, weights, variant))
    rng = np.random.default_rng([N, int(weights)])
    relf = [_t(dev, rng.standard_normal((R1, D))) for _ in range(2)]
    layers = [(_t(dev, rng.standard_normal((D, D)) / np.sqrt(D) * 0.4), _t(dev, 0.1 * rng.standard_normal(D)),
               _t(dev, rng.standard_normal((D, (2 * I + 1) * D)) / np.sqrt((2 * I + 1) * D)),
               _t(dev, 0.1 * rng.standard_normal(D)), None, None) for _ in range(L)]
    w_s, b_s = _t(dev, rng.standard_normal(D) / np.sqrt(D)), _t(dev, [0.1])
    mask = (rng.random(B * N) < 0.8).astype(f32)
    h0 = _t(dev, 0.5 * rng.standard_normal((B * N, D)))
    d0 = rng.random((B, N)) * np.maximum(mask.reshape(B, N), 1e-3)
    d0 = _t(dev, d0 / d0.sum(1, keepdims=True))
    ins = _t(dev, 0.3 * rng.standard_normal((B, I, D)))
    st = ops.LayerStack(plan, relf[0], relf[1], layers, w_s, b_s, _t(dev, mask), I, path=_lib.PATH_FUSED, math=ops.MATH_FP32)
    monkeypatch.setenv("GNNRAG_SOFTMAX_PAIRS", "0")
    two = st.run(h0, d0, ins)
    monkeypatch.delenv("GNNRAG_SOFTMAX_PAIRS")
    st.new_forward()
    one = st.run(h0, d0, ins)
    torch.cuda.synchronize()
    for what, a, b in zip(("h", "score", "dist"), one, two):
        for j in range(L):
            assert torch.equal(a[j], b[j]), "%s of layer %d" % (what, j)
    dist = one[2][L - 1]
    assert torch.isfinite(dist).all() and float((dist.reshape(B, N).sum(1) - 1).abs().max()) < 1e-4


# ---- the recorder ----------------------------------------------------------------------------------------------------------

def record(path=GOLDEN):
    """Writes the golden file.  Run once, with GNNRAG_LIB naming the library of the commit before this module."""
    dev = torch.device("cuda", 0)
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    out = {}
    for R1, D, pos in RT_CASES:
        out[_rt_key(R1, D, pos)] = rt_digests(dev, R1, D, pos)
    for name in STACKS:
        first, second = _stack_runs(name)
        for a, b in zip(first, second):
            assert torch.equal(a, b)
        out["stack_" + name] = stack_digests(first, STACKS[name][4])
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    return out
