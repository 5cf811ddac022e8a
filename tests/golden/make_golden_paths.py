"""Writes tests/golden/paths_ref.npz from the LIVE reference (build machine only: needs the reference checkout and
networkx; no test imports either).

    python tests/golden/make_golden_paths.py --reference /path/to/GNN-RAG [--time]

For every case the fixture holds the batch tuple, seed flags, candidate lists and what the reference's
``build_graph`` + ``get_truth_paths`` (llm/src/utils/graph_utils.py) returned per (seed, candidate) pair, entities named
``str(node id)`` and relations ``str(relation id)``.  The reference module opens ``entities_names.json`` from the working
directory at import: it is imported from a temporary directory that holds an empty one; nothing is written into the
reference tree.

``--time`` reports the reference's own seconds per question (search alone, and with ``build_graph``) on the batches
``tools/time_paths.py`` uses, and writes nothing.
"""
import argparse
import dataclasses
import importlib.util
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import gnnrag_amd  # noqa: E402,F401
from gnnrag_amd import synth  # noqa: E402
import paths_oracle  # noqa: E402


def load_reference(root):
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "entities_names.json"), "w") as f:
        json.dump({}, f)
    cwd = os.getcwd()
    os.chdir(d)
    try:
        spec = importlib.util.spec_from_file_location("ref_graph_utils", os.path.join(root, "llm/src/utils/graph_utils.py"))
        gu = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(gu)
    finally:
        os.chdir(cwd)
    return gu


def question_graph(gu, h, r, t, b, N):
    idx = np.flatnonzero((h // N == b) & (h != t))          # the loader's self-loop facts are not KG triples
    return gu.build_graph([(str(h[i]), str(r[i]), str(t[i])) for i in idx])


def run_case(gu, heads, rels, tails, B, N, R1, seed_flag, cands):
    """cands: per question the candidate slots, best first (caller-made here)."""
    h, r, t = (np.asarray(x, dtype=np.int64) for x in (heads, rels, tails))
    cand_slot = np.full((B, N), -1, dtype=np.int32)
    cand_cnt = np.zeros((B, 2), dtype=np.int32)
    ref_pair, owner, paths = [], [], []
    for b in range(B):
        cand_slot[b, : len(cands[b])] = cands[b]
        cand_cnt[b] = (len(cands[b]), len(cands[b]))
        G = question_graph(gu, h, r, t, b, N)
        for s in np.flatnonzero(seed_flag[b]).tolist():
            for c in cands[b]:
                got = gu.get_truth_paths([str(b * N + s)], [str(b * N + c)], G)
                ref_pair.append((b, s, c, len(got)))
                for p in got:
                    owner.append(len(ref_pair) - 1)
                    paths.append([(int(u), int(x), int(v)) for u, x, v in p])
    L = max([len(p) for p in paths] + [1])
    tri = np.full((len(paths), L, 3), -1, dtype=np.int32)
    for i, p in enumerate(paths):
        if p:
            tri[i, : len(p)] = p
    return {"heads": h.astype(np.int32), "rels": r.astype(np.int32), "tails": t.astype(np.int32),
            "B": np.int32(B), "N": np.int32(N), "R1": np.int32(R1), "seed_flag": np.asarray(seed_flag, dtype=np.uint8),
            "cand_slot": cand_slot, "cand_cnt": cand_cnt, "ref_pair": np.asarray(ref_pair, dtype=np.int32).reshape(-1, 4),
            "ref_path_pair": np.asarray(owner, dtype=np.int32), "ref_paths": tri}


def synth_case(gu, name, B, n_cands, rng):
    cfg = dataclasses.replace(synth.CONFIGS[name], B=B)
    batch = synth.make_batch(cfg)
    h, r, t = batch.edge_tuple[:3]
    seed_flag = (np.asarray(batch.query_entities) == 1).astype(np.uint8)
    cands = []
    for b in range(B):
        n = int(batch.n_real[b])
        pick = rng.choice(n, min(n_cands, n), replace=False).tolist() if n else []
        cands.append([int(x) for x in pick])
    return run_case(gu, h, r, t, B, cfg.N, cfg.R1, seed_flag, cands)


def hand_case(gu, N, facts, seeds, cands, R1=16):
    """One question: facts = [(head, rel, tail)], seeds / cands = slot lists."""
    h, r, t = (np.asarray([f[k] for f in facts], dtype=np.int64) for k in range(3))
    flag = np.zeros((1, N), dtype=np.uint8)
    flag[0, seeds] = 1
    return run_case(gu, h, r, t, 1, N, R1, flag, [list(cands)])


def diamond_chain(n=11):
    facts, cur, nid = [], 0, 1
    for i in range(n):
        a, b, m = nid, nid + 1, nid + 2
        nid += 3
        facts += [(cur, i % 5, a), (b, (i + 1) % 5, cur), (a, (i + 2) % 5, m), (m, (i + 3) % 5, b)]
        cur = m
    return facts, nid, cur


def make_cases(gu):
    rng = np.random.default_rng(5)
    cases = {}
    cases["tiny50"] = synth_case(gu, "tiny50", 4, 8, rng)
    cases["tiny"] = synth_case(gu, "tiny", 3, 8, rng)
    cases["c1x2"] = synth_case(gu, "C1", 2, 10, rng)
    # parallel facts: the later fact wins, also when it is the reversed orientation or sits between other pairs' facts
    cases["parallel"] = hand_case(gu, 8, [(0, 1, 1), (1, 2, 0), (1, 3, 2), (2, 5, 3), (1, 4, 2), (3, 6, 2), (2, 7, 3),
                                          (3, 3, 3), (0, 8, 4), (4, 9, 3), (4, 1, 0), (0, 2, 1), (1, 9, 0)],
                                 [0], [1, 2, 3, 4])
    # slots 0-2 and 3-4 are two components, slot 5 has no fact, slot 6 only a self loop
    cases["unreachable"] = hand_case(gu, 8, [(0, 1, 1), (1, 2, 2), (3, 3, 4), (6, 4, 6)], [0], [2, 4, 5, 6, 1])
    cases["seed_is_cand"] = hand_case(gu, 6, [(0, 1, 1), (1, 2, 2), (0, 3, 2), (2, 1, 3)], [0], [0, 3, 2])
    # a seed without any edge offered as its own candidate: the reference returns nothing
    cases["lonely_seed"] = hand_case(gu, 6, [(1, 1, 2), (2, 2, 3)], [0], [0, 2])
    cases["two_seeds"] = hand_case(gu, 8, [(0, 1, 1), (1, 2, 2), (5, 3, 2), (5, 4, 6), (6, 5, 3), (2, 6, 3), (1, 7, 6)],
                                  [0, 5], [3, 2, 6])
    cases["seed_at_end"] = hand_case(gu, 8, [(7, 1, 1), (1, 2, 2), (7, 3, 3), (3, 4, 2), (2, 5, 6)], [7], [2, 6, 0])
    facts, n, end = diamond_chain(11)
    assert n == 34
    cases["diamonds"] = hand_case(gu, n, facts, [0], [end])
    return cases


def check_against_oracle(cases):
    """The plain-Python restatement must reproduce what was just recorded (the generator refuses to write otherwise)."""
    for name, c in cases.items():
        adj = paths_oracle.adjacency(c["heads"].tolist(), c["tails"].tolist())
        N = int(c["N"])
        for b, s, cs, n, ref in paths_oracle.reference_pairs({k: v for k, v in c.items()}):
            got_n, hops, recs = paths_oracle.pair(adj, b * N + s, b * N + cs)
            assert got_n == n and paths_oracle.as_triples(recs, c["rels"]) == ref, (name, b, s, cs, n, got_n)
            assert [r[0][::-1] for r in recs] == sorted(r[0][::-1] for r in recs), (name, "rank order")


def time_reference(gu, per=4, n_cands=10):
    """Seconds per question of the reference's search on the synthetic shapes (one seed, n_cands random candidates)."""
    rng = np.random.default_rng(7)
    for name in ("C1", "C3", "C2"):
        cfg = dataclasses.replace(synth.CONFIGS[name], B=per)
        batch = synth.make_batch(cfg)
        h, r, t = (np.asarray(x) for x in batch.edge_tuple[:3])
        t_build = t_search = 0.0
        n_paths = 0
        for b in range(per):
            n = int(batch.n_real[b])
            cands = rng.choice(n, min(n_cands, n), replace=False)
            t0 = time.perf_counter()
            G = question_graph(gu, h, r, t, b, cfg.N)
            t1 = time.perf_counter()
            got = gu.get_truth_paths([str(b * cfg.N)], [str(b * cfg.N + int(c)) for c in cands], G)
            t2 = time.perf_counter()
            t_build += t1 - t0
            t_search += t2 - t1
            n_paths += len(got)
        print(json.dumps({"shape": name, "questions": per, "cands": n_cands, "paths_per_question": n_paths / per,
                          "search_ms_per_question": 1e3 * t_search / per,
                          "with_build_graph_ms_per_question": 1e3 * (t_search + t_build) / per}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("GNNRAG_REFERENCE"),
                    help="checkout of the reference (cmavro/GNN-RAG); default: $GNNRAG_REFERENCE")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "paths_ref.npz"))
    a = ap.parse_args()
    if not a.reference:
        ap.error("--reference (or GNNRAG_REFERENCE) must name a checkout of the reference")
    gu = load_reference(a.reference)
    if a.time:
        time_reference(gu)
        return
    cases = make_cases(gu)
    check_against_oracle(cases)
    flat = {"%s/%s" % (n, k): v for n, c in cases.items() for k, v in c.items()}
    np.savez_compressed(a.out, **flat)
    print("wrote", a.out, os.path.getsize(a.out), "bytes;",
          {n: (len(c["ref_pair"]), len(c["ref_paths"])) for n, c in cases.items()})


if __name__ == "__main__":
    main()
