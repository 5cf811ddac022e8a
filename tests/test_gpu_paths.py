"""Reasoning paths on the GPU through the C ABI (gnnrag_ugraph_build + gnnrag_shortest_paths) and the user-facing
``retrieve_paths``: against the fixture recorded from the live reference (tests/golden/paths_ref.npz) and against the
plain-Python restatement (tests/paths_oracle.py) that the CPU tests pin to that fixture.  Integer work: every
comparison is equality."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import paths_oracle

pytestmark = pytest.mark.gpu

CASES = ["tiny50", "tiny", "c1x2", "parallel", "unreachable", "seed_is_cand", "lonely_seed", "two_seeds", "seed_at_end",
         "diamonds"]


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cases():
    return paths_oracle.load_cases()


def _plan(h, r, t, B, N, R1, dev):
    from gnnrag_amd import ops
    return ops.CsrPlan(np.asarray(h, dtype=np.int64), np.asarray(r, dtype=np.int64), np.asarray(t, dtype=np.int64),
                       B, N, R1, dev)


def _call(graph, seed_flag, cand_slot, cand_cnt, S, C, K, H, dev):
    """One gnnrag_shortest_paths call on host inputs; everything copied back (whole worst-case arrays included)."""
    from gnnrag_amd import ops
    sf = torch.from_numpy(np.ascontiguousarray(seed_flag, dtype=np.uint8)).to(dev)
    cs = torch.from_numpy(np.ascontiguousarray(cand_slot, dtype=np.int32)).to(dev)
    cc = torch.from_numpy(np.ascontiguousarray(cand_cnt, dtype=np.int32)).to(dev)
    out = ops.shortest_paths(graph, sf, cs, cc, S, C, K, H)
    return _host(out)


def _host(out):
    off = out.path_off.cpu().numpy()
    total = int(off[-1])
    return {"q_info": out.q_info.cpu().numpy(), "pair_info": out.pair_info.cpu().numpy(), "path_off": off,
            "nodes": out.path_nodes[:total].cpu().numpy(), "facts": out.path_facts[:total].cpu().numpy()}


def _check_against_oracle(got, want, S, C, H):
    q_info, pair_info, records = want
    assert np.array_equal(got["q_info"], q_info)
    assert np.array_equal(got["pair_info"], pair_info)
    B = len(q_info)
    flat = pair_info.reshape(-1, 2)
    assert got["path_off"][0] == 0 and len(got["path_off"]) == B * S * C + 1
    for p in range(B * S * C):
        recs = records.get(p, [])
        have = paths_oracle.device_records(got["path_off"], got["nodes"], got["facts"], p, max(int(flat[p, 1]), 0))
        assert have == recs, p                                  # the oracle's ranks 0 .. k-1, in rank order
    # -1 padding behind every record
    for r in range(len(got["nodes"])):
        h = int((got["nodes"][r] >= 0).sum()) - 1
        assert (got["nodes"][r, h + 1:] == -1).all() and (got["facts"][r, h:] == -1).all() and (got["facts"][r, :h] >= 0).all()


@pytest.mark.parametrize("name", CASES)
def test_fixture_cases_equal_the_reference(dev, cases, name):
    from gnnrag_amd import ops
    c = cases[name]
    B, N, R1 = int(c["B"]), int(c["N"]), int(c["R1"])
    graph = ops.UGraph.from_plan(_plan(c["heads"], c["rels"], c["tails"], B, N, R1, dev))
    S, C, K, H = 2, 16, 4096, 32
    got = _call(graph, c["seed_flag"], c["cand_slot"], c["cand_cnt"], S, C, K, H, dev)
    seeds = [np.flatnonzero(c["seed_flag"][b]).tolist() for b in range(B)]
    ref = paths_oracle.reference_pairs(c)
    assert len(ref) == sum(len(seeds[b]) * int(c["cand_cnt"][b, 1]) for b in range(B))
    seen = 0
    for b, s, cs, n, want in ref:
        si = seeds[b].index(s)
        ci = c["cand_slot"][b].tolist().index(cs)
        p = (b * S + si) * C + ci
        n_got, hops = got["pair_info"][b, si, ci].tolist()
        assert n_got == n, (name, b, s, cs)
        assert (hops == -1) == (n == 0)
        recs = paths_oracle.device_records(got["path_off"], got["nodes"], got["facts"], p, max(hops, 0))
        assert len(recs) == n and all(nd[0] == b * N + s and nd[-1] == b * N + cs for nd, _ in recs)
        assert paths_oracle.as_triples(recs, c["rels"]) == want, (name, b, s, cs)        # nodes and relations, as sets
        seen += n
    assert seen == got["path_off"][-1]
    # and against the restatement: hops, q_info, rank order, padding
    _check_against_oracle(got, paths_oracle.batch(c["heads"], c["tails"], B, N, c["seed_flag"], c["cand_slot"],
                                                  c["cand_cnt"], S, C, K, H), S, C, H)


def _adjacency_equal(graph, h, t, BN):
    got = graph.to_host()
    u_ptr, u_adj = paths_oracle.ugraph_numpy(h, t, BN)
    assert np.array_equal(got["u_ptr"], u_ptr)
    assert np.array_equal(got["u_adj"], u_adj)


def test_adjacency_from_a_built_structure(dev, cases):
    from gnnrag_amd import ops, synth
    for name in ("tiny", "c1x2", "parallel"):
        c = cases[name]
        B, N = int(c["B"]), int(c["N"])
        plan = _plan(c["heads"], c["rels"], c["tails"], B, N, int(c["R1"]), dev)
        _adjacency_equal(ops.UGraph.from_plan(plan), c["heads"], c["tails"], B * N)
    # the non-waiting build (relation counts passed in)
    cfg = synth.CONFIGS["tiny"]
    batch = synth.make_batch(cfg)
    h, r, t = batch.edge_tuple[:3]
    counts = [len(set(r[(h // cfg.N) == b].tolist())) for b in range(cfg.B)]
    plan = ops.CsrPlan(h, r, t, cfg.B, cfg.N, cfg.R1, dev, rel_counts=(sum(counts), max(counts)))
    graph = ops.UGraph.from_plan(plan)
    plan.status()
    _adjacency_equal(graph, h, t, cfg.B * cfg.N)


def test_adjacency_from_a_concatenated_structure(dev, cases):
    from gnnrag_amd import ops
    c = cases["tiny50"]
    B, N, R1 = int(c["B"]), int(c["N"]), int(c["R1"])
    h, r, t = (c[k].astype(np.int64) for k in ("heads", "rels", "tails"))
    q = h // N
    assert (np.diff(q) >= 0).all()                              # the questions' facts are contiguous, in batch order
    parts = [_plan(h[q == b] - b * N, r[q == b], t[q == b] - b * N, 1, N, R1, dev) for b in range(B)]
    plan = ops.CsrPlan.concat(parts, N, R1, dev)
    graph = ops.UGraph.from_plan(plan)
    _adjacency_equal(graph, h, t, B * N)
    got = _call(graph, c["seed_flag"], c["cand_slot"], c["cand_cnt"], 2, 16, 64, 8, dev)
    _check_against_oracle(got, paths_oracle.batch(h, t, B, N, c["seed_flag"], c["cand_slot"], c["cand_cnt"], 2, 16, 64, 8),
                          2, 16, 8)


def test_adjacency_from_a_hub_sorted_structure(dev):
    """Relation vocabulary above the hub-sort threshold of csr_plan.hip, rows heavier than heavy_deg: hub rows are in
    (relation, fact id) order there, the adjacency must not assume fact order."""
    from gnnrag_amd import ops
    from test_gpu_hub_rows import _graph
    B, N, R, h, r, t = _graph()
    plan = ops.CsrPlan(h, r, t, B, N, R, dev)
    host = plan.to_host()
    assert int(plan.c.hub_sorted) == 1 and host["n_heavy"][0] >= 1 and host["n_heavy"][1] >= 3
    graph = ops.UGraph.from_plan(plan)
    _adjacency_equal(graph, h, t, B * N)
    # paths through the hubs: seeds = the hub nodes, candidates = random nodes
    rng = np.random.default_rng(11)
    seed_flag = np.zeros((B, N), dtype=np.uint8)
    seed_flag[0, 5], seed_flag[0, 7], seed_flag[1, 9], seed_flag[2, 100] = 1, 1, 1, 1
    cand_slot = np.full((B, N), -1, dtype=np.int32)
    cand_slot[:, :12] = rng.integers(0, N, (B, 12))
    cand_cnt = np.full((B, 2), 12, dtype=np.int32)
    S, C, K, H = 2, 12, 2048, 16
    want = paths_oracle.batch(h, t, B, N, seed_flag, cand_slot, cand_cnt, S, C, K, H)
    assert want[1][..., 0].max() <= K
    _check_against_oracle(_call(graph, seed_flag, cand_slot, cand_cnt, S, C, K, H, dev), want, S, C, H)


def _peaked_pred(rng, batch):
    """Seeded random distribution whose top-p cut retrieves a handful of candidates per question: a few eligible slots
    share 0.97 of the mass, the others the rest."""
    B, N = batch.local_entity.shape
    p = np.zeros((B, N), dtype=np.float64)
    for b in range(B):
        n = int(batch.n_real[b])
        if n < 2:
            continue
        k = int(rng.integers(3, 11))
        top = rng.choice(np.arange(1, n), min(k, n - 1), replace=False)
        p[b, :n] = 0.03 * rng.dirichlet(np.ones(n))
        p[b, top] += 0.97 * rng.dirichlet(np.ones(len(top)) * 4.0)
    return p.astype(np.float32)


SWEEP = [("C1", 1, 3), ("C1", 1, 4), ("C3", 32, 5), ("C2", 8, 6)]


@pytest.mark.parametrize("shape,B,seed", SWEEP, ids=["%s-B%d-s%d" % s for s in SWEEP])
def test_random_sweep_exact_and_cut(dev, shape, B, seed):
    from gnnrag_amd import ops, synth
    cfg = dataclasses.replace(synth.CONFIGS[shape], B=B)
    batch = synth.make_batch(cfg, seed=seed)
    h, r, t = batch.edge_tuple[:3]
    N = cfg.N
    graph = ops.UGraph.from_plan(ops.CsrPlan(h, r, t, B, N, cfg.R1, dev))
    rng = np.random.default_rng(100 + seed)
    pred = torch.from_numpy(_peaked_pred(rng, batch)).to(dev)
    seeds = batch.query_entities == 1
    eligible = (~seeds) & (batch.local_entity != batch.num_entity)
    eps = 0.95
    slots, cnt = ops.topp_candidates(pred, torch.from_numpy(eligible.astype(np.uint8)).to(dev), (1 - eps) / N, eps)
    sf = torch.from_numpy(seeds.astype(np.uint8)).to(dev)
    slots_h, cnt_h = slots.cpu().numpy(), cnt.cpu().numpy()
    # exact: the limits cut nothing - a condition on the inputs, asserted from the oracle before equality is demanded
    S, C, K, H = 2, 16, 1024, 16
    want = paths_oracle.batch(h, t, B, N, seeds, slots_h, cnt_h, S, C, K, None)
    assert want[0][:, 0].max() <= S and 1 <= want[0][:, 1].max() <= C
    assert want[1][..., 0].max() <= K and want[1][..., 1].max() <= H
    print("sweep %s B=%d: pairs with paths %d, max n_paths %d, max hops %d, records %d" % (
        shape, B, int((want[1][..., 0] > 0).sum()), int(want[1][..., 0].max()), int(want[1][..., 1].max()),
        sum(len(v) for v in want[2].values())))
    _check_against_oracle(_host(ops.shortest_paths(graph, sf, slots, cnt, S, C, K, H)), want, S, C, H)
    # cut: n_paths stays the true count, the records are the oracle's ranks 0 .. 3 in order
    got = _host(ops.shortest_paths(graph, sf, slots, cnt, S, C, 4, H))
    cut = paths_oracle.batch(h, t, B, N, seeds, slots_h, cnt_h, S, C, 4, H)
    assert np.array_equal(cut[1], want[1])
    _check_against_oracle(got, cut, S, C, H)
    for p, recs in want[2].items():
        assert cut[2][p] == recs[:4]


BIG = [("wide", 65536, 150000), ("dense", 8192, 400000)]


@pytest.mark.parametrize("name,N,E", BIG, ids=[b[0] for b in BIG])
def test_large_questions(dev, name, N, E):
    """wide: the largest supported question (65536 node slots: the levels fill 64 KiB of LDS).  dense: every node has more
    neighbours than a lane scans and there are more such rows than the wave list holds, so both the wave-scanned rows and
    the lane fallback behind the list run."""
    from gnnrag_amd import ops
    rng = np.random.default_rng(N)
    B = 2
    h = np.concatenate([rng.integers(0, N, E) + b * N for b in range(B)])
    t = np.concatenate([rng.integers(0, N, E) + b * N for b in range(B)])
    r = rng.integers(0, 20, B * E)
    graph = ops.UGraph.from_plan(ops.CsrPlan(h, r, t, B, N, 22, dev))
    _adjacency_equal(graph, h, t, B * N)
    seed_flag = np.zeros((B, N), dtype=np.uint8)
    seed_flag[0, [3, N - 1]] = 1
    seed_flag[1, N // 2] = 1
    cand_slot = np.full((B, N), -1, dtype=np.int32)
    cand_slot[:, :8] = rng.integers(0, N, (B, 8))
    cand_cnt = np.full((B, 2), 8, dtype=np.int32)
    S, C, K, H = 2, 8, 256, 16
    want = paths_oracle.batch(h, t, B, N, seed_flag, cand_slot, cand_cnt, S, C, K, H)
    assert (want[1][..., 0] > 0).sum() >= 8
    if name == "dense":
        u_ptr = graph.to_host()["u_ptr"]
        assert (np.diff(u_ptr)[:N] > 32).sum() > 4096
    _check_against_oracle(_call(graph, seed_flag, cand_slot, cand_cnt, S, C, K, H, dev), want, S, C, H)


def test_diamond_chain_limits(dev, cases):
    from gnnrag_amd import ops
    c = cases["diamonds"]
    graph = ops.UGraph.from_plan(_plan(c["heads"], c["rels"], c["tails"], 1, 34, int(c["R1"]), dev))
    adj = paths_oracle.adjacency(c["heads"].tolist(), c["tails"].tolist())
    n, hops, ranked = paths_oracle.pair(adj, 0, 33)
    assert (n, hops, len(ranked)) == (2048, 22, 2048)
    args = (graph, c["seed_flag"], c["cand_slot"], c["cand_cnt"])
    got = _call(*args, 1, 1, 8, 32, dev)
    assert got["pair_info"].reshape(-1).tolist() == [2048, 22] and got["path_off"].tolist() == [0, 8]
    assert paths_oracle.device_records(got["path_off"], got["nodes"], got["facts"], 0, 22) == ranked[:8]
    got = _call(*args, 1, 1, 4096, 32, dev)
    assert got["pair_info"].reshape(-1).tolist() == [2048, 22] and got["path_off"].tolist() == [0, 2048]
    recs = paths_oracle.device_records(got["path_off"], got["nodes"], got["facts"], 0, 22)
    assert recs == ranked
    (_, _, _, n_ref, want), = paths_oracle.reference_pairs(c)
    assert n_ref == 2048 and paths_oracle.as_triples(recs, c["rels"]) == want
    got = _call(*args, 1, 1, 8, 8, dev)
    assert got["pair_info"].reshape(-1).tolist() == [0, -1] and got["path_off"].tolist() == [0, 0] and len(got["nodes"]) == 0


def test_path_count_saturates(dev):
    """32 diamonds: 2^32 shortest paths of 64 hops.  n_paths saturates at INT32_MAX and the ranks below max_paths are
    still the right ones (the unranking only compares ranks below max_paths with the saturated counts)."""
    from gnnrag_amd import ops
    h, t, cur, nid = [], [], 0, 1
    for _ in range(32):
        a, b, m = nid, nid + 1, nid + 2
        nid += 3
        h += [cur, b, a, m]
        t += [a, cur, m, b]
        cur = m
    N = nid
    graph = ops.UGraph.from_plan(_plan(h, [0] * len(h), t, 1, N, 4, dev))
    seed_flag = np.zeros((1, N), dtype=np.uint8)
    seed_flag[0, 0] = 1
    cand_slot = np.full((1, N), -1, dtype=np.int32)
    cand_slot[0, :2] = (cur, cur - 3)
    cand_cnt = np.array([[2, 2]], dtype=np.int32)
    want = paths_oracle.batch(h, t, 1, N, seed_flag, cand_slot, cand_cnt, 1, 2, 4, 64)
    assert want[1][0, 0].tolist() == [[2 ** 31 - 1, 64], [2 ** 31 - 1, 62]] and len(want[2][0]) == 4
    _check_against_oracle(_call(graph, seed_flag, cand_slot, cand_cnt, 1, 2, 4, 64, dev), want, 1, 2, 64)


def _raw_buffers(graph, sf, cs, cc, S, C, K, H, fill):
    """Worst-case buffers pre-filled with `fill`, then one call: what the call wrote is what differs from the fill."""
    from gnnrag_amd import ops
    buf = ops.PathBuffers(graph.B, graph.N, S, C, K, H, graph.device)
    for x in (buf.q_info, buf.pair_info, buf.path_off, buf.path_nodes, buf.path_facts):
        x.fill_(fill)
    ops.shortest_paths(graph, sf, cs, cc, S, C, K, H, buffers=buf)
    return [x.cpu().numpy() for x in (buf.q_info, buf.pair_info, buf.path_off, buf.path_nodes, buf.path_facts)]


def test_reproducible_and_position_independent(dev, cases):
    from gnnrag_amd import ops
    c = cases["c1x2"]
    N, R1 = 2000, int(c["R1"])
    h, r, t = (c[k].astype(np.int64) for k in ("heads", "rels", "tails"))
    graph = ops.UGraph.from_plan(_plan(h, r, t, 2, N, R1, dev))
    sf = torch.from_numpy(c["seed_flag"]).to(dev)
    cs = torch.from_numpy(c["cand_slot"]).to(dev)
    cc = torch.from_numpy(c["cand_cnt"]).to(dev)
    S, C, K, H = 2, 16, 64, 8
    a = _raw_buffers(graph, sf, cs, cc, S, C, K, H, -7)
    b = _raw_buffers(graph, sf, cs, cc, S, C, K, H, -7)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)                              # whole buffers, bit for bit
    total = int(a[2][-1])
    assert total > 0 and (a[3][total:] == -7).all() and (a[4][total:] == -7).all()      # compact: nothing behind the prefix
    # question 1 alone, as question 0 of its own batch
    own = (h // N) == 1
    f0 = int(np.flatnonzero(own)[0])
    assert np.array_equal(np.flatnonzero(own), np.arange(f0, f0 + own.sum()))
    g1 = ops.UGraph.from_plan(_plan(h[own] - N, r[own], t[own] - N, 1, N, R1, dev))
    one = _raw_buffers(g1, sf[1:2].contiguous(), cs[1:2].contiguous(), cc[1:2].contiguous(), S, C, K, H, -7)
    P1 = S * C
    assert np.array_equal(one[0], a[0][1:2]) and np.array_equal(one[1], a[1][1:2])
    o = a[2][P1:] - a[2][P1]
    assert np.array_equal(one[2], o)
    n1 = int(one[2][-1])
    nodes = a[3][a[2][P1]: a[2][P1] + n1]
    facts = a[4][a[2][P1]: a[2][P1] + n1]
    assert n1 > 0 and np.array_equal(one[3][:n1], np.where(nodes >= 0, nodes - N, -1))
    assert np.array_equal(one[4][:n1], np.where(facts >= 0, facts - f0, -1))


def test_selection_then_paths_without_a_wait(dev):
    """gnnrag_topp_candidates -> gnnrag_shortest_paths enqueued back to back on one stream (the candidate lists never
    leave the device) equals the two-step form with a host round trip in between."""
    from gnnrag_amd import ops, synth
    cfg = dataclasses.replace(synth.CONFIGS["C3"], B=4)
    batch = synth.make_batch(cfg, seed=9)
    h, r, t = batch.edge_tuple[:3]
    graph = ops.UGraph.from_plan(ops.CsrPlan(h, r, t, cfg.B, cfg.N, cfg.R1, dev))
    pred = torch.from_numpy(_peaked_pred(np.random.default_rng(21), batch)).to(dev)
    seeds = batch.query_entities == 1
    el = torch.from_numpy(((~seeds) & (batch.local_entity != batch.num_entity)).astype(np.uint8)).to(dev)
    sf = torch.from_numpy(seeds.astype(np.uint8)).to(dev)
    S, C, K, H = 2, 16, 64, 8
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        slots, cnt = ops.topp_candidates(pred, el, 0.05 / cfg.N, 0.95)
        buf = ops.PathBuffers(cfg.B, cfg.N, S, C, K, H, dev)
        ops.shortest_paths(graph, sf, slots, cnt, S, C, K, H, buffers=buf)          # no wait in between
    stream.synchronize()
    chained = _host(buf)
    slots_h, cnt_h = slots.cpu().numpy(), cnt.cpu().numpy()
    two = _call(graph, seeds, slots_h, cnt_h, S, C, K, H, dev)
    for k in chained:
        assert np.array_equal(chained[k], two[k]), k
    assert chained["path_off"][-1] > 0
    _check_against_oracle(chained, paths_oracle.batch(h, t, cfg.B, cfg.N, seeds, slots_h, cnt_h, S, C, K, H), S, C, H)


def test_retrieve_paths_on_the_closed_loop_batches(dev):
    from gnnrag_amd import eval_tail, ops, paths
    z = np.load(os.path.join(GOLDEN, "rearev_closed_loop.npz"))
    N = int(z["max_local_entity"])
    eps = float(z["eps"])
    ignore_prob = (1 - eps) / N
    id2entity = {i: str(s) for i, s in enumerate(z["id2entity"])}
    pad = len(id2entity)
    S, C, K, H = 4, 16, 64, 8
    with_paths = 0
    for k in range(int(z["n_batches"])):
        g = lambda name: z["b%d.%s" % (k, name)]
        h, r, t = g("heads"), g("rels"), g("tails")
        le, qe = g("local_entity"), g("query_entities")
        B = le.shape[0]
        plan = ops.CsrPlan(h, r, t, B, N, int(z["num_kb_relation"]) + 1, dev)
        pred = torch.from_numpy(g("pred_dist")).to(dev)
        got, info = paths.retrieve_paths(plan, r, pred, le, qe, pad, ignore_prob, eps, S, C, K, H, return_info=True)
        picked = eval_tail.retrieved_candidates(pred, le, qe, pad, ignore_prob, eps)
        adj = paths_oracle.adjacency(h.tolist(), t.tolist())
        records = 0
        for b in range(B):
            cands = [e for e, _ in picked[b][0]]
            seeds = np.flatnonzero(qe[b].astype(np.int64) == 1)
            assert info[b].tolist() == [len(seeds), len(cands)] and len(seeds) <= S
            assert len(got[b]) == len(seeds) * min(len(cands), C)
            for i, pr in enumerate(got[b]):
                s, ci = seeds[i // min(len(cands), C)], i % min(len(cands), C)
                assert pr["cand"] == cands[ci] and pr["seed_slot"] == s and pr["seed"] == le[b, s]
                n, hops, recs = paths_oracle.pair(adj, b * N + int(s), b * N + pr["cand_slot"], K, H)
                assert (pr["n_paths"], pr["hops"]) == (n, hops)
                want = [[(int(le[b, nd[j] - b * N]), int(r[fc[j]]), int(le[b, nd[j + 1] - b * N])) for j in range(len(fc))]
                        for nd, fc in recs]
                assert pr["paths"] == want
                records += len(recs)
                with_paths += n > 0
        # the readback is the fixed blocks plus the records that exist - not the padded cube
        rb = paths.LAST_READBACK
        P = B * S * C
        assert rb["records"] == records and rb["record_bytes"] == records * (2 * H + 1) * 4
        assert rb["fixed_bytes"] == (2 * B + 2 * P + P + 1 + B * C) * 4
        # names instead of ids, rendered as the reference renders a path for the LLM
        names = dict(id2entity)
        names[pad] = "<pad>"
        relname = {i: "r%d" % i for i in range(int(z["num_kb_relation"]) + 1)}
        named = paths.retrieve_paths(plan, r, pred, le, qe, pad, ignore_prob, eps, S, C, K, H, id2entity=names,
                                     id2relation=relname)
        for b in range(B):
            for a, nm in zip(got[b], named[b]):
                assert nm["seed"] == names[a["seed"]] and nm["cand"] == names[a["cand"]]
                for pa, pn in zip(a["paths"], nm["paths"]):
                    assert pn == [(names[u], relname[x], names[v]) for u, x, v in pa]
                    want = " -> ".join([names[pa[0][0]]] + [y for _, x, v in pa for y in (relname[x], names[v])]) if pa else ""
                    assert paths.path_to_string(pn) == want
    assert with_paths > 0
