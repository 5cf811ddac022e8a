"""CPU-side checks of the rule-guided walks: the plain-Python restatement (tests/rule_paths_oracle.py) against the fixture
recorded from the live reference (tests/golden/rule_paths_ref.npz), the host-only ``reasoning_context``, the three entry
points in header and binding, and the argument checks of ``retrieve_rule_paths`` that need no device."""
import os
import re
import types

import numpy as np
import pytest

from conftest import REPO

import rule_paths_oracle

CASES = ["tiny50", "tiny", "c1x2", "back_and_forth", "winning_relation", "lonely_seed", "two_seeds", "unknown_relation",
         "hub", "k44", "ragged"]
S, R, K, H = 4, 8, 64, 4                    # the defaults of ops.rule_paths; the fixture's rule arrays are [B, 8, 4]


@pytest.fixture(scope="module")
def cases():
    return rule_paths_oracle.load_cases()


def test_fixture_holds_every_case(cases):
    assert sorted(cases) == sorted(CASES)


@pytest.mark.parametrize("name", CASES)
def test_oracle_equals_the_reference(cases, name):
    c = cases[name]
    B, N = int(c["B"]), int(c["N"])
    assert c["rule_rel"].shape == (B, R, H) and c["rule_len"].shape == (B, R)
    q_info, pair_info, records = rule_paths_oracle.batch(c["heads"], c["rels"], c["tails"], B, N, c["seed_flag"],
                                                         c["rule_rel"], c["rule_len"], S, R, K, H)
    seeds = [np.flatnonzero(c["seed_flag"][b]).tolist() for b in range(B)]
    valid = (c["rule_len"] >= 1) & (c["rule_len"] <= H)
    assert q_info.tolist() == [[len(seeds[b]), int(valid[b].sum())] for b in range(B)]
    assert q_info[:, 0].max() <= S                                           # nothing is cut at the default limits
    ref = rule_paths_oracle.reference_pairs(c)
    assert len(ref) == sum(len(seeds[b]) * int(valid[b].sum()) for b in range(B))      # every existing pair is recorded
    seen = set()
    for b, s, k, n, want in ref:
        si = seeds[b].index(s)
        p = (b * S + si) * R + k
        seen.add(p)
        assert pair_info[b, si, k].tolist() == [n, int(c["rule_len"][b, k])], (name, b, s, k)
        walks = records[p]
        assert n <= K and len(walks) == n == len(want)
        assert all(nd[0] == b * N + s and len(nd) == len(fc) + 1 == c["rule_len"][b, k] + 1 for nd, fc in walks)
        triples = {tuple((nd[i], int(c["rels"][fc[i]]), nd[i + 1]) for i in range(len(fc))) for nd, fc in walks}
        assert triples == want, (name, b, s, k)
        assert [nd for nd, _ in walks] == sorted(nd for nd, _ in walks)        # ascending rank order, no duplicates
        assert all(r == int(x) for nd, fc in walks for r, x in zip(c["rule_rel"][b, k], c["rels"][list(fc)]))
    for p in range(B * S * R):                                               # the slots that do not exist
        if p not in seen:
            assert pair_info.reshape(-1, 2)[p].tolist() == [0, -1] and not records.get(p)


def test_hand_made_expectations(cases):
    def counts(name):
        return {(b, s, k): n for b, s, k, n, _ in rule_paths_oracle.reference_pairs(cases[name])}

    c = counts("back_and_forth")
    assert c[(0, 0, 0)] == 8
    walks = rule_paths_oracle.reference_pairs(cases["back_and_forth"])[0][4]
    assert ((0, 1, 1), (1, 1, 0), (0, 1, 1)) in walks                         # 0 -> 1 -> 0 -> 1: back over the same edge
    w = counts("winning_relation")                                           # rules [1] [2] [9] [8] [9,4] [9,4,7] [1,9] [9,3]
    assert [w[(0, 0, k)] for k in range(8)] == [1, 0, 1, 0, 1, 1, 1, 0]
    ref = rule_paths_oracle.reference_pairs(cases["winning_relation"])
    assert ref[0][4] == {((0, 1, 4),)} and ref[2][4] == {((0, 9, 1),)}        # both won by a fact of reversed orientation
    assert set(counts("lonely_seed").values()) == {0}
    assert [n for (_, _, k), n in sorted(counts("unknown_relation").items()) if k < 5] == [0] * 10
    assert counts("k44")[(0, 0, 0)] == 64
    h = cases["hub"]
    deg = np.bincount(np.concatenate([h["heads"], h["tails"]]), minlength=48)
    assert deg[0] == 40 and len(set(h["rels"][(h["heads"] == 0) | (h["tails"] == 0)].tolist())) == 3
    assert cases["ragged"]["rule_len"][0].tolist()[:5] == [0, 1, H, H + 1, 2] and not cases["ragged"]["seed_flag"][1].any()


def _process_input_lists(rule_paths, shortest_paths, path_to_string):
    """build_qa_input.py:105-123 restated literally on lists of paths."""
    lists_of_paths = []
    if len(rule_paths) > 0:
        lists_of_paths = [path_to_string(p) for p in rule_paths]
    for p in shortest_paths:
        if path_to_string(p) not in lists_of_paths:
            lists_of_paths.append(path_to_string(p))
    return lists_of_paths


def test_reasoning_context_is_the_union_of_process_input():
    from gnnrag_amd import paths
    a = [("q", "r1", "x"), ("x", "r2", "y")]
    b = [("q", "r1", "x"), ("x", "r1", "q")]
    c = [("q", "r3", "z")]
    d = [("q", "r1", "x")]
    rule = [{"paths": [a, b]}, {"paths": []}, {"paths": [d]}]
    short = [{"paths": [d, c]}, {"paths": [c, a]}]               # d and a are present already, c comes twice
    got = paths.reasoning_context(rule, short)
    want = _process_input_lists([a, b, d], [d, c, c, a], paths.path_to_string)
    assert got == want == ["q -> r1 -> x -> r2 -> y", "q -> r1 -> x -> r1 -> q", "q -> r1 -> x", "q -> r3 -> z"]
    assert paths.reasoning_context([], short) == _process_input_lists([], [d, c, c, a], paths.path_to_string)
    assert paths.reasoning_context(rule, None) == [paths.path_to_string(p) for p in (a, b, d)]
    assert paths.reasoning_context(None, None) == []
    # a rule path is kept even when it repeats (only the shortest paths are filtered)
    assert paths.reasoning_context([{"paths": [d, d]}], [{"paths": [d]}]) == ["q -> r1 -> x"] * 2


NEW = {"gnnrag_rule_paths_workspace_bytes": 5, "gnnrag_rule_paths_out_bytes": 5, "gnnrag_rule_paths": 17}


def test_header_and_binding_declare_the_entry_points():
    from gnnrag_amd import _lib
    src = open(os.path.join(REPO, "include", "gnnrag.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, n_args in NEW.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, "gnnrag.h does not declare " + name
        assert len(m.group(1).split(",")) == n_args
        assert name in _lib.SIGNATURES, "the binding lacks " + name
        assert len(_lib.SIGNATURES[name][1]) == n_args
    assert re.search(r"#define\s+GNNRAG_ABI_VERSION\s+16\b", src) and _lib.ABI_VERSION == 16


def test_library_exports_the_entry_points_and_sizes():
    from gnnrag_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)
    # erel [2 F] int32 + down [B][rules][hops][N] uint32, each rounded up to 256 bytes - and nothing else
    F, B, N = 768000, 64, 2000
    ws = lib.gnnrag_rule_paths_workspace_bytes(F, B, N, 8, 4)
    assert 2 * F * 4 + B * 8 * 4 * N * 4 <= ws <= 2 * F * 4 + B * 8 * 4 * N * 4 + 512
    assert lib.gnnrag_rule_paths_workspace_bytes(0, 1, 1, 1, 1) == 512
    for bad in ((-1, B, N, 8, 4), (F, 0, N, 8, 4), (F, B, 0, 8, 4), (F, B, N, 0, 4), (F, B, N, 8, 0), (F, B, N, 8, 255),
                (F, B, 65537, 8, 4), (2 ** 30, B, N, 8, 4), (F, 2 ** 20, 65536, 8, 4)):
        assert lib.gnnrag_rule_paths_workspace_bytes(*bad) == 0, bad
    assert lib.gnnrag_rule_paths_workspace_bytes(F, B, 65536, 8, 254) > 0
    assert lib.gnnrag_rule_paths_out_bytes(B, 4, 8, 64, 4) == lib.gnnrag_paths_out_bytes(B, 4, 8, 64, 4) > 0
    assert lib.gnnrag_rule_paths_out_bytes(B, 4, 8, 64, 255) == 0 and lib.gnnrag_rule_paths_out_bytes(B, 4, 8, 0, 4) == 0
    assert lib.gnnrag_rule_paths_out_bytes(2 ** 15, 2 ** 8, 2 ** 8, 1, 4) == 0           # P * max_paths >= 2^31
    assert lib.gnnrag_rule_paths_out_bytes(2 ** 10, 4, 8, 2 ** 16, 4) == 0
    # bad arguments are refused before anything touches a device
    assert lib.gnnrag_rule_paths(None, None, None, None, None, 4, 8, 64, 4, None, None, None, None, None, None, 0, None) == -1


def test_retrieve_rule_paths_refuses_rules_beyond_the_limits():
    """Raised from the host-side packing, before any device work: a stand-in for the plan is enough."""
    from gnnrag_amd import paths
    plan = types.SimpleNamespace(B=2, N=5)
    le = qe = np.zeros((2, 5))
    with pytest.raises(ValueError, match="max_rules"):
        paths.retrieve_rule_paths(plan, [], le, qe, [[[1]] * 3, []], max_rules=2)
    with pytest.raises(ValueError, match="max_hops"):
        paths.retrieve_rule_paths(plan, [], le, qe, [[[1, 2, 3]], []], max_hops=2)
    with pytest.raises(ValueError, match="per question"):
        paths.retrieve_rule_paths(plan, [], le, qe, [[[1]]])
    rel, ln = paths._pack_rules([[["a", "b"], ["zz"]], [[]]], 2, {"a": 3, "b": 5}, 3, 2)
    assert rel[0].tolist() == [[3, 5], [-1, -1], [-1, -1]] and ln.tolist() == [[2, 1, 0], [0, 0, 0]]
