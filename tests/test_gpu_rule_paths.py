"""Rule-guided walks on the GPU through the C ABI (gnnrag_rule_paths) and the user-facing ``retrieve_rule_paths``:
against the fixture recorded from the live reference (tests/golden/rule_paths_ref.npz) and against the plain-Python
restatement (tests/rule_paths_oracle.py) that the CPU tests pin to that fixture.  Integer work: every comparison is
equality."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import paths_oracle
import rule_paths_oracle

pytestmark = pytest.mark.gpu

CASES = ["tiny50", "tiny", "c1x2", "back_and_forth", "winning_relation", "lonely_seed", "two_seeds", "unknown_relation",
         "hub", "k44", "ragged"]
INT32_MAX = 2 ** 31 - 1
FILL = -7


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cases():
    return rule_paths_oracle.load_cases()


def _plan(h, r, t, B, N, R1, dev):
    from gnnrag_amd import ops
    return ops.CsrPlan(np.asarray(h, dtype=np.int64), np.asarray(r, dtype=np.int64), np.asarray(t, dtype=np.int64),
                       B, N, R1, dev)


def _dev(dev, rels, seed_flag, rule_rel, rule_len):
    return (torch.from_numpy(np.ascontiguousarray(rels, dtype=np.int32)).to(dev),
            torch.from_numpy(np.ascontiguousarray(seed_flag, dtype=np.uint8)).to(dev),
            torch.from_numpy(np.ascontiguousarray(rule_rel, dtype=np.int32)).to(dev),
            torch.from_numpy(np.ascontiguousarray(rule_len, dtype=np.int32)).to(dev))


def _host(out):
    off = out.path_off.cpu().numpy()
    total = int(off[-1])
    return {"q_info": out.q_info.cpu().numpy(), "pair_info": out.pair_info.cpu().numpy(), "path_off": off,
            "nodes": out.path_nodes[:total].cpu().numpy(), "facts": out.path_facts[:total].cpu().numpy()}


def _call(graph, rels, seed_flag, rule_rel, rule_len, S, R, K, H, dev):
    """One gnnrag_rule_paths call on host inputs; the fixed blocks and the record prefix copied back."""
    from gnnrag_amd import ops
    return _host(ops.rule_paths(graph, *_dev(dev, rels, seed_flag, rule_rel, rule_len), S, R, K, H))


def _raw(graph, args, S, R, K, H, fill=FILL):
    """Worst-case buffers pre-filled with ``fill``, then one call: everything copied back, whole arrays."""
    from gnnrag_amd import ops
    buf = ops.RulePathBuffers(graph.F, graph.B, graph.N, S, R, K, H, graph.device)
    outs = (buf.q_info, buf.pair_info, buf.path_off, buf.path_nodes, buf.path_facts)
    for x in outs:
        x.fill_(fill)
    buf.ws.fill_(fill & 0xFF)
    ops.rule_paths(graph, *args, S, R, K, H, buffers=buf)
    return [x.cpu().numpy() for x in outs]


def _check_against_oracle(got, want, S, R, H):
    q_info, pair_info, records = want
    assert np.array_equal(got["q_info"], q_info)
    assert np.array_equal(got["pair_info"], pair_info)
    B = len(q_info)
    flat = pair_info.reshape(-1, 2)
    assert got["path_off"][0] == 0 and len(got["path_off"]) == B * S * R + 1
    for p in range(B * S * R):
        have = paths_oracle.device_records(got["path_off"], got["nodes"], got["facts"], p, max(int(flat[p, 1]), 0))
        assert have == records.get(p, []), p                     # the oracle's ranks 0 .. k-1, in rank order
    assert got["path_off"][-1] == len(got["nodes"]) == len(got["facts"]) == sum(len(v) for v in records.values())
    for p in range(B * S * R):                                   # -1 padding behind every record's hops
        h = max(int(flat[p, 1]), 0)
        rows = slice(int(got["path_off"][p]), int(got["path_off"][p + 1]))
        assert (got["nodes"][rows, h + 1:] == -1).all() and (got["facts"][rows, h:] == -1).all()
        assert (got["nodes"][rows, : h + 1] >= 0).all() and (got["facts"][rows, :h] >= 0).all()


def _oracle(h, r, t, B, N, seed_flag, rule_rel, rule_len, S, R, K, H):
    return rule_paths_oracle.batch(h, r, t, B, N, seed_flag, rule_rel, rule_len, S, R, K, H)


def _pack(rules, B, R, H):
    from gnnrag_amd import paths
    return paths._pack_rules(rules, B, None, R, H)


@pytest.mark.parametrize("name", CASES)
def test_fixture_cases_equal_the_reference(dev, cases, name):
    from gnnrag_amd import ops
    c = cases[name]
    B, N, R1 = int(c["B"]), int(c["N"]), int(c["R1"])
    graph = ops.UGraph.from_plan(_plan(c["heads"], c["rels"], c["tails"], B, N, R1, dev))
    S, R, K, H = 4, 8, 64, 4                                    # the defaults: the fixture is cut nowhere
    got = _call(graph, c["rels"], c["seed_flag"], c["rule_rel"], c["rule_len"], S, R, K, H, dev)
    seeds = [np.flatnonzero(c["seed_flag"][b]).tolist() for b in range(B)]
    valid = (c["rule_len"] >= 1) & (c["rule_len"] <= H)
    assert got["q_info"].tolist() == [[len(seeds[b]), int(valid[b].sum())] for b in range(B)]
    assert got["q_info"][:, 0].max() <= S and got["pair_info"][..., 0].max() <= K          # no cut
    ref = rule_paths_oracle.reference_pairs(c)
    assert len(ref) == sum(len(seeds[b]) * int(valid[b].sum()) for b in range(B))
    seen, records = set(), 0
    for b, s, k, n, want in ref:
        si = seeds[b].index(s)
        p = (b * S + si) * R + k
        seen.add(p)
        assert got["pair_info"][b, si, k].tolist() == [n, int(c["rule_len"][b, k])], (name, b, s, k)
        recs = paths_oracle.device_records(got["path_off"], got["nodes"], got["facts"], p, int(c["rule_len"][b, k]))
        assert len(recs) == n and all(nd[0] == b * N + s for nd, _ in recs)
        assert paths_oracle.as_triples(recs, c["rels"]) == want, (name, b, s, k)           # nodes and relations, as sets
        records += n
    flat = got["pair_info"].reshape(-1, 2)
    for p in range(B * S * R):                                   # every other slot: no seed of that index, or no rule
        if p not in seen:
            assert flat[p].tolist() == [0, -1] and got["path_off"][p] == got["path_off"][p + 1], (name, p)
    assert records == got["path_off"][-1]
    # and against the restatement, exactly: q_info, pair_info, path_off, the records in rank order, the padding
    _check_against_oracle(got, _oracle(c["heads"], c["rels"], c["tails"], B, N, c["seed_flag"], c["rule_rel"],
                                       c["rule_len"], S, R, K, H), S, R, H)


def test_cut_keeps_the_count_and_the_first_ranks(dev, cases):
    from gnnrag_amd import ops
    c = cases["k44"]
    graph = ops.UGraph.from_plan(_plan(c["heads"], c["rels"], c["tails"], 1, 8, int(c["R1"]), dev))
    S, R, K, H = 4, 8, 5, 4
    want = _oracle(c["heads"], c["rels"], c["tails"], 1, 8, c["seed_flag"], c["rule_rel"], c["rule_len"], S, R, None, H)
    assert want[1][0, 0, 0].tolist() == [64, 3] and len(want[2][0]) == 64 and want[1][0, 0, 1].tolist() == [16, 2]
    q_info, pair_info, off, nodes, facts = _raw(graph, _dev(dev, c["rels"], c["seed_flag"], c["rule_rel"], c["rule_len"]),
                                                S, R, K, H)
    assert np.array_equal(pair_info, want[1])                    # n_paths stays the true count
    assert off[:3].tolist() == [0, 5, 10]                        # the following pair starts directly behind
    total = int(off[-1])
    assert total == 20                                           # 2 seeds x 2 rules, 5 records each
    for p in (0, 1, R, R + 1):
        h = int(pair_info.reshape(-1, 2)[p, 1])
        assert paths_oracle.device_records(off, nodes, facts, p, h) == want[2][p][:5]
    assert (nodes[total:] == FILL).all() and (facts[total:] == FILL).all()      # nothing behind path_off[P] is touched


def test_walk_count_saturates(dev):
    """Complete bipartite 32 + 32, one relation, a rule of 7 hops: 32^7 > 2^31 walks from every node.  n_paths saturates
    at INT32_MAX and the first max_paths records are the oracle's.  Checked against the oracle only: the reference
    enumerates its walks one by one and cannot produce 3 * 10^10 of them."""
    from gnnrag_amd import ops
    N = 64
    h = np.repeat(np.arange(32), 32)
    t = np.tile(np.arange(32, 64), 32)
    r = np.full(len(h), 3)
    graph = ops.UGraph.from_plan(_plan(h, r, t, 1, N, 8, dev))
    seed_flag = np.zeros((1, N), dtype=np.uint8)
    seed_flag[0, [0, 40]] = 1
    rule_rel, rule_len = _pack([[[3] * 7, [3] * 6]], 1, 2, 7)
    S, R, K, H = 2, 2, 64, 7
    want = _oracle(h, r, t, 1, N, seed_flag, rule_rel, rule_len, S, R, K, H)
    assert want[1][0].tolist() == [[[INT32_MAX, 7], [2 ** 30, 6]]] * 2 and [len(want[2][p]) for p in range(4)] == [64] * 4
    _check_against_oracle(_call(graph, r, seed_flag, rule_rel, rule_len, S, R, K, H, dev), want, S, R, H)


def _sweep_batch(shape, B, seed, extra_seeds=3, n_rules=8, max_len=3):
    from gnnrag_amd import synth
    cfg = dataclasses.replace(synth.CONFIGS[shape], B=B)
    batch = synth.make_batch(cfg, seed=seed)
    h, r, t = batch.edge_tuple[:3]
    rng = np.random.default_rng(1000 + seed)
    seed_flag = (batch.query_entities == 1).astype(np.uint8)
    for b in range(B):
        n = int(batch.n_real[b])
        if n > 1:
            seed_flag[b, rng.choice(np.arange(1, n), min(extra_seeds, n - 1), replace=False)] = 1
    rules = synth.sample_rules(h, r, t, B, cfg.N, seed_flag, n_rules, max_len, rng, n_rel=cfg.R)
    return cfg, h, r, t, seed_flag, rules


@pytest.mark.parametrize("shape,B,seed", [("tiny50", 5, 31), ("C1", 3, 32)])
def test_random_sweep_exact_and_cut(dev, shape, B, seed):
    from gnnrag_amd import ops
    cfg, h, r, t, seed_flag, rules = _sweep_batch(shape, B, seed)
    N = cfg.N
    graph = ops.UGraph.from_plan(ops.CsrPlan(h, r, t, B, N, cfg.R1, dev))
    S, R, K, H = 4, 8, 64, 4
    rule_rel, rule_len = _pack(rules, B, R, H)
    want = _oracle(h, r, t, B, N, seed_flag, rule_rel, rule_len, S, R, K, H)
    assert want[0][:, 0].max() == S and want[0][:, 1].max() == R and 3 <= want[1][..., 0].max() <= K
    print("sweep %s B=%d: pairs with walks %d of %d, max n_paths %d, records %d" % (
        shape, B, int((want[1][..., 0] > 0).sum()), int((want[1][..., 1] > 0).sum()), int(want[1][..., 0].max()),
        sum(len(v) for v in want[2].values())))
    _check_against_oracle(_call(graph, r, seed_flag, rule_rel, rule_len, S, R, K, H, dev), want, S, R, H)
    # limits below what the data holds: 2 of 4 seeds, the first 5 of 8 rules, 2 records per pair
    S2, R2, K2 = 2, 5, 2
    rr2, rl2 = np.ascontiguousarray(rule_rel[:, :R2]), np.ascontiguousarray(rule_len[:, :R2])
    cut = _oracle(h, r, t, B, N, seed_flag, rr2, rl2, S2, R2, K2, H)
    assert cut[0][:, 0].max() > S2 and cut[1][..., 0].max() > K2               # both cuts are there to be seen
    assert np.array_equal(cut[1], want[1][:, :S2, :R2])                          # counts are the true ones
    raw = _raw(graph, _dev(dev, r, seed_flag, rr2, rl2), S2, R2, K2, H)
    total = int(raw[2][-1])
    got = {"q_info": raw[0], "pair_info": raw[1], "path_off": raw[2], "nodes": raw[3][:total], "facts": raw[4][:total]}
    _check_against_oracle(got, cut, S2, R2, H)
    assert (got["q_info"][:, 0] > S2).any() and (got["pair_info"][..., 0] > K2).any()
    for p, recs in cut[2].items():
        b, si, k = p // (S2 * R2), p // R2 % S2, p % R2
        assert recs == want[2][(b * S + si) * R + k][:K2]
    assert (raw[3][total:] == FILL).all() and (raw[4][total:] == FILL).all()    # nothing written out of place


def test_large_question(dev):
    """One question of 20000 node slots and 100000 edges with Zipf heads: rows far heavier than a lane scans, levels
    summed by whole waves, counts beyond max_paths."""
    from gnnrag_amd import ops, synth
    cfg = synth.GraphConfig(name="big", B=1, N=20000, E=100000, R=40, D=8, I=1, L=1)
    batch = synth.make_batch(cfg, seed=77)
    h, r, t = batch.edge_tuple[:3]
    rng = np.random.default_rng(78)
    seed_flag = (batch.query_entities == 1).astype(np.uint8)
    seed_flag[0, [1, 19999]] = 1                                 # slot 1: the heaviest Zipf head
    rules = synth.sample_rules(h, r, t, 1, cfg.N, seed_flag, 4, 3, rng, n_rel=cfg.R)
    graph = ops.UGraph.from_plan(ops.CsrPlan(h, r, t, 1, cfg.N, cfg.R1, dev))
    assert (np.diff(graph.to_host()["u_ptr"]) > 32).sum() >= 8
    S, R, K, H = 3, 4, 64, 3
    rule_rel, rule_len = _pack(rules, 1, R, H)
    want = _oracle(h, r, t, 1, cfg.N, seed_flag, rule_rel, rule_len, S, R, K, H)
    assert (want[1][..., 0] > 0).sum() >= 3 and want[1][..., 0].max() > K
    _check_against_oracle(_call(graph, r, seed_flag, rule_rel, rule_len, S, R, K, H, dev), want, S, R, H)


def test_same_result_from_built_concatenated_and_hub_sorted_structures(dev):
    """Relation vocabulary above the hub-sort threshold of csr_plan.hip (R1 > 1024), rows heavier than heavy_deg: the
    built structure has its hub rows in (relation, fact id) order, the concatenated one is made of per-question parts."""
    from gnnrag_amd import ops, synth
    from test_gpu_hub_rows import _graph
    B, N, Rv, h, r, t = _graph()
    order = np.argsort(h // N, kind="stable")                    # the questions' facts contiguous, in batch order
    h, r, t = h[order], r[order], t[order]
    q = h // N
    built = ops.CsrPlan(h, r, t, B, N, Rv, dev)
    host = built.to_host()
    assert Rv > 1024 and int(built.c.hub_sorted) == 1 and host["n_heavy"][0] >= 1 and host["n_heavy"][1] >= 3
    parts = [_plan(h[q == b] - b * N, r[q == b], t[q == b] - b * N, 1, N, Rv, dev) for b in range(B)]
    concat = ops.CsrPlan.concat(parts, N, Rv, dev)
    seed_flag = np.zeros((B, N), dtype=np.uint8)
    seed_flag[0, [5, 6, 7]], seed_flag[1, 9], seed_flag[2, 100] = 1, 1, 1      # the hub nodes
    rules = synth.sample_rules(h, r, t, B, N, seed_flag, 8, 2, np.random.default_rng(12), n_rel=Rv)
    rules[0][0] = [7]                                            # the 3000-fact relation of node 5
    S, R, K, H = 3, 8, 64, 2
    rule_rel, rule_len = _pack(rules, B, R, H)
    want = _oracle(h, r, t, B, N, seed_flag, rule_rel, rule_len, S, R, K, H)
    assert want[1][0, 0, 0, 0] > 1000 and (want[1][..., 0] > 0).sum() >= 10
    results = []
    for plan in (built, concat):
        got = _call(ops.UGraph.from_plan(plan), r, seed_flag, rule_rel, rule_len, S, R, K, H, dev)
        _check_against_oracle(got, want, S, R, H)
        results.append(got)
    for k in results[0]:
        assert np.array_equal(results[0][k], results[1][k]), k


def test_reproducible_and_position_independent(dev, cases):
    from gnnrag_amd import ops
    c = cases["tiny"]
    B, N, R1 = int(c["B"]), int(c["N"]), int(c["R1"])
    h, r, t = (c[k].astype(np.int64) for k in ("heads", "rels", "tails"))
    graph = ops.UGraph.from_plan(_plan(h, r, t, B, N, R1, dev))
    S, R, K, H = 4, 8, 64, 4
    args = _dev(dev, r, c["seed_flag"], c["rule_rel"], c["rule_len"])
    a = _raw(graph, args, S, R, K, H)
    b = _raw(graph, args, S, R, K, H, fill=0x55)
    for i, (x, y) in enumerate(zip(a, b)):
        total = int(a[2][-1]) if i >= 3 else len(x)
        assert np.array_equal(x[:total], y[:total]), i            # bit for bit, whatever the buffers held
    total = int(a[2][-1])
    assert total > 0 and (a[3][total:] == FILL).all() and (a[4][total:] == FILL).all()
    # question 2 alone, as question 0 of its own batch
    own = (h // N) == 2
    f0 = int(np.flatnonzero(own)[0])
    assert np.array_equal(np.flatnonzero(own), np.arange(f0, f0 + own.sum()))
    g1 = ops.UGraph.from_plan(_plan(h[own] - 2 * N, r[own], t[own] - 2 * N, 1, N, R1, dev))
    one = _raw(g1, _dev(dev, r[own], c["seed_flag"][2:3], c["rule_rel"][2:3], c["rule_len"][2:3]), S, R, K, H)
    P1 = 2 * S * R
    assert np.array_equal(one[0], a[0][2:3]) and np.array_equal(one[1], a[1][2:3])
    assert np.array_equal(one[2], a[2][P1:] - a[2][P1])
    n1 = int(one[2][-1])
    nodes = a[3][a[2][P1]: a[2][P1] + n1]
    facts = a[4][a[2][P1]: a[2][P1] + n1]
    assert n1 > 0 and np.array_equal(one[3][:n1], np.where(nodes >= 0, nodes - 2 * N, -1))
    assert np.array_equal(one[4][:n1], np.where(facts >= 0, facts - f0, -1))


def test_pipeline_on_the_closed_loop_batches(dev):
    """retrieve_rule_paths + retrieve_paths + reasoning_context: the strings of the union equal those built from the two
    restatements the way build_qa_input.py:105-123 builds them."""
    from gnnrag_amd import eval_tail, ops, paths, synth
    z = np.load(os.path.join(GOLDEN, "rearev_closed_loop.npz"))
    N = int(z["max_local_entity"])
    eps = float(z["eps"])
    ignore_prob = (1 - eps) / N
    pad = len(z["id2entity"])
    S, R, K, H = 4, 8, 64, 3
    C, H2 = 16, 8
    rule_strings = dropped = 0
    for k in range(int(z["n_batches"])):
        g = lambda name: z["b%d.%s" % (k, name)]
        h, r, t = g("heads"), g("rels"), g("tails")
        le, qe = g("local_entity"), g("query_entities")
        B = le.shape[0]
        seeds = qe.astype(np.int64) == 1
        rules = synth.sample_rules(h, r, t, B, N, seeds, R, H, np.random.default_rng(40 + k))
        plan = ops.CsrPlan(h, r, t, B, N, int(z["num_kb_relation"]) + 1, dev)
        graph = ops.UGraph.from_plan(plan)
        pred = torch.from_numpy(g("pred_dist")).to(dev)
        got_short = paths.retrieve_paths(graph, r, pred, le, qe, pad, ignore_prob, eps, S, C, K, H2)
        for b in range(B):                                       # one rule that is the relation path of a shortest path
            known = [p for x in got_short[b] for p in x["paths"] if 1 <= len(p) <= H]
            if known:
                rules[b][-1] = [int(x) for _, x, _ in known[0]]
        got_rule, info = paths.retrieve_rule_paths(graph, r, le, qe, rules, None, S, R, K, H, return_info=True)
        rb = dict(paths.LAST_RULE_READBACK)
        picked = eval_tail.retrieved_candidates(pred, le, qe, pad, ignore_prob, eps)
        by_rel = rule_paths_oracle.rel_adjacency(h, r, t)
        adj = paths_oracle.adjacency(h.tolist(), t.tolist())

        def triples(b, nd, fc):
            return [(int(le[b, nd[j] - b * N]), int(r[fc[j]]), int(le[b, nd[j + 1] - b * N])) for j in range(len(fc))]

        records = 0
        for b in range(B):
            slots = np.flatnonzero(seeds[b])[:S].tolist()
            assert info[b].tolist() == [int(seeds[b].sum()), len(rules[b])]
            assert len(got_rule[b]) == len(slots) * len(rules[b])
            want_rule, i = [], 0
            for s in slots:
                for rule in rules[b]:
                    n, walks = rule_paths_oracle.pair(by_rel, b * N + s, rule, K)
                    pr = got_rule[b][i]
                    i += 1
                    assert (pr["seed_slot"], pr["seed"], pr["rule"], pr["n_paths"], pr["hops"]) == \
                        (s, le[b, s], rule, n, len(rule))
                    assert pr["paths"] == [triples(b, nd, fc) for nd, fc in walks]
                    want_rule += pr["paths"]
                    records += len(walks)
            want_short = []
            n_c = min(len(picked[b][0]), C)
            assert len(got_short[b]) == len(slots) * n_c
            for si, s in enumerate(slots):
                for ci in range(n_c):
                    pr = got_short[b][si * n_c + ci]
                    assert pr["cand"] == picked[b][0][ci][0] and pr["seed_slot"] == s
                    _, _, recs = paths_oracle.pair(adj, b * N + s, b * N + pr["cand_slot"], K, H2)
                    want_short += [triples(b, nd, fc) for nd, fc in recs]
            want = [paths.path_to_string(p) for p in want_rule]                  # build_qa_input.py:105-123
            for p in want_short:
                if paths.path_to_string(p) not in want:
                    want.append(paths.path_to_string(p))
            assert paths.reasoning_context(got_rule[b], got_short[b]) == want
            rule_strings += len(want_rule)
            dropped += len(want_rule) + len(want_short) - len(want)
        P = B * S * R
        assert rb["records"] == records and rb["record_bytes"] == records * (2 * H + 1) * 4
        assert rb["fixed_bytes"] == (2 * B + 2 * P + P + 1) * 4
    assert rule_strings > 0 and dropped > 0                     # shortest paths the rule walks had found already
