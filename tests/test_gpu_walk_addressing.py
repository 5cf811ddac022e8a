"""The LDS walk (k_walk_slice), held to the bytes of the library before its global addressing and its guarded loads were
rewritten (32-bit lane offsets from uniform bases, unconditional clamped loads with a select, row pointers requested a set
ahead and consumed a set later): tests/golden/walk_slice_parent.json names the commit whose library wrote the digests.

Tuples come from tests/walk_probe.py's ``build_graph``; the data is full mantissa (priors = softmax of 6 N(0, 1), N(0, 1)
tables, weights in [0.5, 1.5)), so a fact that is dropped, doubled, read from a neighbour's run or added in another order
changes the bytes.  No case is at the workload's shape.  What the cases cover:

* B = 3, 9 (every item cut in two) and 41 (full rounds plus a split tail), B % 8 != 0; B = 1 at N = 1028 (pl = 2);
* N = 100 and 1028 (no multiple of 16: the last set is partial);
* D = 200 and 20 on the 16-column kernels (13 slices; 2 slices, the second 4 columns wide), D = 72 on the 32-column ones;
* rows of 0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 65 and 4097 facts at node slots 0 and N - 1 - question q puts LENS[q % 14]
  at slot 0 and LENS[(q + 7) % 14] at slot N - 1, in direction (q // 14) % 2 and the other one, so that B = 41 has every
  length at both slots in both directions and B = 3 / 9 a prefix of them; the same lengths again on both sides of a set
  boundary, and as merged runs (a, b);
* a question without facts, and one with more than 72 big nodes (no big-node list: lane groups walk every row);
* with and without per-fact weights;
* both directions in one call (``ops.aggregate_fused``: the merged-row instantiations, digest of ``nbr``) and each
  direction alone (GNNRAG_PATH_ONLY_FWD / _INV of ``ops.reason_layer``, the only way to the instantiations without merged
  rows and to their skip_dir; there ``nbr`` stays inside the call, the digest is over h_out, score and dist_out).

Every case first asserts the walk variant it reaches; two calls return the same bytes.  The digests were recorded by
``record()`` below, run once with GNNRAG_LIB pointing at the parent commit's build; they are never regenerated from the
code under test.
"""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import walk_probe as wp

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "walk_slice_parent.json")
LENS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 65, 4097)


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


def _question(q, nrel):
    """Rows of question q: LENS[q % 14] at slot 0 in direction (q // 14) % 2, LENS[(q + 7) % 14] at slot N - 1 in the other
    one, the same two lengths on both sides of the first set boundary (slots 15, 16) with the directions swapped, then
    merged runs."""
    a, b = LENS[q % 14], LENS[(q + 7) % 14]
    d = (q // 14) % 2
    row = (lambda l, d: (l, 0) if d == 0 else (0, l))
    place = [row(a, d), row(b, 1 - d), row(b, d), row(a, 1 - d)]
    big = max(a, b) > 33
    place += [(min(a, 65), min(b, 65)), (8, 1), (1, 8), (9, 8), (16, 17)]
    # a 4097-fact row needs few sinks, or every node of the question turns big; they then hold medium rows
    return dict(place=place, nrel=nrel, sinks=(30 if big else None), extra=120)


@functools.lru_cache(maxsize=None)
def graph(name):
    if name in ("q3", "q3_r60"):
        # question 0: the ladder, every relation; question 1: no facts; question 2: 73 rows of 33 facts whose sources are the
        # 27 other nodes (they turn big as well): more big nodes than the list holds
        R = 320 if name == "q3" else 60
        q0 = dict(_question(6, None), extra=R + 100)
        q2 = dict(place=[(33, i % 3) for i in range(73)], nrel=17)
        g = wp.build_graph(name, 3, 100, R, [q0, None, q2], seed=41)
        assert len(g.big_nodes(2)) > wp.BIG_CAP and g.len0[100:200].sum() == 0 and g.len1[100:200].sum() == 0
        return g
    if name in ("q9", "q41"):
        B = int(name[1:])
        qs = [dict(_question(q, None if q == 0 else 1 + q % 17), extra=(420 if q == 0 else 120)) for q in range(B)]
        return wp.build_graph(name, B, 100, 320, qs, seed=42 + B)
    if name == "q1_n1028":
        place = [(4097, 0), (0, 4097)] + [(l, 0) for l in LENS[1:13]] + [(0, l) for l in LENS[1:13]] + [(65, 64), (8, 8)]
        g = wp.build_graph(name, 1, 1028, 320, [dict(place=place, nrel=None, sinks=60, extra=2500)], seed=44)
        assert len(g.big_nodes(0)) <= wp.BIG_CAP            # the list exists: the 4097-fact rows go to the whole workgroup
        return g
    raise KeyError(name)


# name: (graph, D, weights, what: "both" or the one direction walked, walk variant, launch regime at 256 CUs or None)
CASES = {
    "q3_d200": ("q3", 200, False, "both", wp.WALK_LDS_16, "every item split"),
    "q3_d200_w": ("q3", 200, True, "both", wp.WALK_LDS_16, "every item split"),
    "q3_d20": ("q3", 20, False, "both", wp.WALK_LDS_16, "every item split"),
    "q3_r60_d72": ("q3_r60", 72, False, "both", wp.WALK_LDS_32, "every item split"),
    "q3_r60_d72_w": ("q3_r60", 72, True, "both", wp.WALK_LDS_32, "every item split"),
    "q9_d200": ("q9", 200, False, "both", wp.WALK_LDS_16, "every item split"),
    "q9_d20_w": ("q9", 20, True, "both", wp.WALK_LDS_16, "every item split"),
    "q41_d200": ("q41", 200, False, "both", wp.WALK_LDS_16, "full rounds plus a split tail"),
    "q41_d200_w": ("q41", 200, True, "both", wp.WALK_LDS_16, "full rounds plus a split tail"),
    "q1_n1028_d200": ("q1_n1028", 200, False, "both", wp.WALK_LDS_16, "pl=2"),
    "q1_n1028_d200_w": ("q1_n1028", 200, True, "both", wp.WALK_LDS_16, "pl=2"),
    "q3_d200_fwd": ("q3", 200, False, 0, wp.WALK_LDS_16, None),
    "q3_d200_inv_w": ("q3", 200, True, 1, wp.WALK_LDS_16, None),
    "q9_d200_inv": ("q9", 200, False, 1, wp.WALK_LDS_16, None),
    "q9_d200_fwd_w": ("q9", 200, True, 0, wp.WALK_LDS_16, None),
    "q3_r60_d72_fwd_w": ("q3_r60", 72, True, 0, wp.WALK_LDS_32, None),
    "q3_r60_d72_inv": ("q3_r60", 72, False, 1, wp.WALK_LDS_32, None),
}


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def run_case(name, dev):
    """The digests of two calls of the case, after the assertions on the form it reaches."""
    from gnnrag_amd import _lib, ops
    gname, D, wts, what, variant, regime = CASES[name]
    g = graph(gname)
    rng = np.random.default_rng(sum(map(ord, name)) * 8 + 5)
    dist = wp.random_priors(g, rng)
    w = (0.5 + rng.random(g.F)).astype(np.float32) if wts else None
    plan = ops.CsrPlan(g.h, g.r, g.t, g.B, g.N, g.R, dev)
    assert plan.rel_total == g.rel_total
    if w is not None:
        plan.attach_w_gnn(w)
    assert ops.aggregate_fused_variant(plan, D) == variant == wp.walk_variant(g.rel_max, D), name
    if regime is not None:
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        reg = wp.launch_regime(g.B, g.N, D, variant, cus)
        if cus == 256:
            assert reg["regime"] == regime, (name, reg)
    if what == "both":
        P = _t(dev, rng.standard_normal((2, g.rel_total, D)))
        d_dist = _t(dev, dist)
        return [_sha(ops.aggregate_fused(plan, d_dist, P)) for _ in range(2)]
    n = lambda *s: _t(dev, rng.standard_normal(s) * 0.1)
    args = (plan, n(g.B * g.N, D), _t(dev, dist), n(g.B, 1, D), n(g.R, D), n(g.R, D), n(D, D), n(D), n(D, 3 * D), n(D), n(D),
            n(1), torch.ones(g.B, g.N, device=dev))
    flag = _lib.PATH_ONLY_INV if what else _lib.PATH_ONLY_FWD
    return [_sha(*ops.reason_layer(*args, path=_lib.PATH_FUSED | flag)) for _ in range(2)]


@pytest.mark.parametrize("name", list(CASES))
def test_walk_bytes_are_the_parents(dev, name):
    first, again = run_case(name, dev)
    assert first == again, name + ": two calls differ"
    assert first == _golden()["digests"][name], name + ": not the bytes the parent's library wrote"


def test_the_ladder_reaches_both_slots():
    """Host only: the row lengths the cases claim, at slots 0 and N - 1 of the B = 41 graph, in both directions."""
    g = graph("q41")
    for slot in (0, g.N - 1):
        nodes = np.arange(g.B) * g.N + slot
        assert set(LENS) <= set(g.len0[nodes].tolist()) and set(LENS) <= set(g.len1[nodes].tolist()), slot


def record(path, commit):
    """Writes the golden file; run once with GNNRAG_LIB naming the build of ``commit``."""
    dev = torch.device("cuda", 0)
    out = {"parent_commit": commit, "device": torch.cuda.get_device_name(0), "digests": {}}
    for name in CASES:
        first, again = run_case(name, dev)
        assert first == again, name
        out["digests"][name] = first
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
