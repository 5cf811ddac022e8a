"""Writes tests/golden/rule_paths_ref.npz from the LIVE reference (build machine only: needs the reference checkout and
networkx; no test imports either).

    python tests/golden/make_golden_rule_paths.py --reference /path/to/GNN-RAG [--time [--time-out FILE]]

For every case the fixture holds the batch tuple, seed flags, the rules (``rule_rel`` [B, 8, 4], ``rule_len`` [B, 8]) and
what the reference's ``build_graph`` + ``bfs_with_rule`` (llm/src/utils/graph_utils.py) returned per (seed, rule) pair in
the loops of ``apply_rules``, entities named ``str(node id)`` and relations ``str(relation id)``.  Only rules of 1 .. 4 hops
are given to the reference: a slot whose ``rule_len`` lies outside is an empty or rejected slot of the C ABI (the
reference answers an EMPTY rule with one empty path, which carries no triple and is dropped by ``direct_answer``).  Rules
are per question (``predicted_paths``): the synthetic cases sample 8 of them per question, from the question's seeds in
turn (``gnnrag_amd.synth.sample_rules``).  The reference module is loaded as ``make_golden_paths.py`` loads it; nothing
of its text is copied.

``--time`` reports the reference's own milliseconds per question for ``bfs_with_rule`` (search alone, and with
``build_graph``) on the batches and rules of ``tools/time_paths.py --rules``; with ``--time-out`` the lines are also
written to that file.  It writes no fixture.
"""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))

from make_golden_paths import load_reference, question_graph  # noqa: E402  (also puts the repository on sys.path)
from gnnrag_amd import synth  # noqa: E402
import rule_paths_oracle  # noqa: E402

R_SLOTS, H_SLOTS = 8, 4          # the defaults of ops.rule_paths: nothing in the fixture is cut there
TIME_SEED = 1234                 # tools/time_paths.py --rules samples its rules with the same seed


def run_case(gu, heads, rels, tails, B, N, R1, seed_flag, rules, lens=None):
    """rules[b]: the question's rules (relation-id lists); lens[b][k] overrides the stated length of slot k."""
    h, r, t = (np.asarray(x, dtype=np.int64) for x in (heads, rels, tails))
    rule_rel = np.full((B, R_SLOTS, H_SLOTS), -1, dtype=np.int32)
    rule_len = np.zeros((B, R_SLOTS), dtype=np.int32)
    ref_pair, owner, paths = [], [], []
    for b in range(B):
        assert len(rules[b]) <= R_SLOTS
        for k, rule in enumerate(rules[b]):
            rule_rel[b, k, : min(len(rule), H_SLOTS)] = rule[:H_SLOTS]
            rule_len[b, k] = len(rule) if lens is None or lens[b][k] is None else lens[b][k]
        G = question_graph(gu, h, r, t, b, N)
        for s in np.flatnonzero(seed_flag[b]).tolist():
            for k, rule in enumerate(rules[b]):
                if not 1 <= rule_len[b, k] <= H_SLOTS:
                    continue
                assert rule_len[b, k] == len(rule)
                got = gu.bfs_with_rule(G, str(b * N + s), [str(x) for x in rule])
                walks = [tuple((int(u), int(x), int(v)) for u, x, v in p) for p in got]
                assert len(set(walks)) == len(walks)              # a simple graph: a walk is its node sequence
                ref_pair.append((b, s, k, len(walks)))
                for p in walks:
                    owner.append(len(ref_pair) - 1)
                    paths.append(p)
    tri = np.full((len(paths), H_SLOTS, 3), -1, dtype=np.int32)
    for i, p in enumerate(paths):
        tri[i, : len(p)] = p
    return {"heads": h.astype(np.int32), "rels": r.astype(np.int32), "tails": t.astype(np.int32),
            "B": np.int32(B), "N": np.int32(N), "R1": np.int32(R1), "seed_flag": np.asarray(seed_flag, dtype=np.uint8),
            "rule_rel": rule_rel, "rule_len": rule_len, "ref_pair": np.asarray(ref_pair, dtype=np.int32).reshape(-1, 4),
            "ref_path_pair": np.asarray(owner, dtype=np.int32), "ref_paths": tri}


def synth_batch(name, B, rng, extra_seeds=3, seed=None):
    """The synthetic batch, its seed flags (the batch's own seed plus up to ``extra_seeds`` random real nodes per
    question) and 8 sampled rules per question of 1 .. 3 hops."""
    cfg = dataclasses.replace(synth.CONFIGS[name], B=B)
    batch = synth.make_batch(cfg, seed=seed)
    h, r, t = batch.edge_tuple[:3]
    seed_flag = (np.asarray(batch.query_entities) == 1).astype(np.uint8)
    for b in range(B):
        n = int(batch.n_real[b])
        if n > 1:
            seed_flag[b, rng.choice(np.arange(1, n), min(extra_seeds, n - 1), replace=False)] = 1
    rules = synth.sample_rules(h, r, t, B, cfg.N, seed_flag, R_SLOTS, 3, rng, n_rel=cfg.R)
    return cfg, h, r, t, seed_flag, rules


def hand_case(gu, N, facts, seeds, rules, R1=16, lens=None):
    """One question: facts = [(head, rel, tail)], seeds = slot list, rules = relation-id lists."""
    h, r, t = (np.asarray([f[k] for f in facts], dtype=np.int64) for k in range(3))
    flag = np.zeros((1, N), dtype=np.uint8)
    flag[0, seeds] = 1
    return run_case(gu, h, r, t, 1, N, R1, flag, [rules], None if lens is None else [lens])


PARALLEL = [(0, 1, 1), (1, 2, 0), (1, 3, 2), (2, 5, 3), (1, 4, 2), (3, 6, 2), (2, 7, 3), (3, 3, 3), (0, 8, 4), (4, 9, 3),
            (4, 1, 0), (0, 2, 1), (1, 9, 0)]          # the facts of make_golden_paths.py's "parallel" case


def make_cases(gu):
    rng = np.random.default_rng(11)
    cases = {}
    for key, name, B in (("tiny50", "tiny50", 4), ("tiny", "tiny", 3), ("c1x2", "C1", 2)):
        cfg, h, r, t, seed_flag, rules = synth_batch(name, B, rng)
        cases[key] = run_case(gu, h, r, t, B, cfg.N, cfg.R1, seed_flag, rules)
    # the triangle 0-1-2 of relation 1 with the tail 1-3 of relation 2: [1,1,1] from 0 has 8 walks, 0 1 0 1 among them
    cases["back_and_forth"] = hand_case(gu, 4, [(0, 1, 1), (1, 1, 2), (2, 1, 0), (1, 2, 3)], [0],
                                        [[1, 1, 1], [1, 1, 2], [1, 2], [2], [1, 2, 2, 1]])
    # winning relations: {0,1} -> 9 (fact 12, reversed), {1,2} -> 4, {2,3} -> 7, {0,4} -> 1 (fact 10, reversed), {3,4} -> 9
    cases["winning_relation"] = hand_case(gu, 8, PARALLEL, [0],
                                          [[1], [2], [9], [8], [9, 4], [9, 4, 7], [1, 9], [9, 3]])
    # slot 0 has no fact, slot 4 only a self loop
    cases["lonely_seed"] = hand_case(gu, 6, [(1, 1, 2), (2, 2, 3), (4, 3, 4)], [0, 4], [[1], [3], [1, 2], [2, 1]])
    cases["two_seeds"] = hand_case(gu, 8, [(0, 1, 1), (1, 2, 2), (5, 3, 2), (5, 4, 6), (6, 5, 3), (2, 6, 3), (1, 7, 6)],
                                   [0, 5], [[1], [3], [1, 2], [3, 2], [4, 5], [3, 6], [4, 7, 1], [2]])
    cases["unknown_relation"] = hand_case(gu, 5, [(0, 1, 1), (1, 2, 2), (2, 1, 3)], [0, 2],
                                          [[99], [-1], [1, 99], [-1, 1], [1, -1], [1], [1, 2], [2, 1, -1]])
    # node 0 has 40 neighbours under 3 relations: its row is summed by a whole wave
    hub = [(0, i % 3 + 1, i) if i % 2 else (i, i % 3 + 1, 0) for i in range(1, 41)]
    hub += [(41, 4, 1), (42, 4, 2), (41, 5, 42), (43, 4, 44), (2, 1, 1)]
    cases["hub"] = hand_case(gu, 48, hub, [0, 5, 41],
                             [[3, 1], [3, 2], [5, 4, 3], [4, 2, 1], [3, 1, 1], [1, 1], [4, 2], [2, 1, 1]])
    k44 = [(a, 1, b) for a in range(4) for b in range(4, 8)]
    cases["k44"] = hand_case(gu, 8, k44, [0, 5], [[1, 1, 1], [1, 1]])
    # rule_len 0, 1, max_hops and max_hops + 1 in one row; question 1 has no seed at all
    h, r, t = zip(*([(0, 1, 1), (1, 1, 2), (2, 1, 3), (3, 1, 4), (4, 1, 0)] + [(6 + a, 1, 6 + b) for a, b in ((0, 1), (1, 2))]))
    flag = np.zeros((2, 6), dtype=np.uint8)
    flag[0, [0, 2]] = 1
    rag = [[[], [1], [1, 1, 1, 1], [1, 1, 1, 1], [1, 1]], [[1], [1, 1]]]
    cases["ragged"] = run_case(gu, h, r, t, 2, 6, 16, flag, rag, lens=[[0, None, None, 5, None], [None, None]])
    return cases


def check_against_oracle(cases):
    """The plain-Python restatement must reproduce what was just recorded (the generator refuses to write otherwise)."""
    stats = {}
    for name, c in cases.items():
        by_rel = rule_paths_oracle.rel_adjacency(c["heads"], c["rels"], c["tails"])
        N = int(c["N"])
        nonempty = 0
        for b, s, k, n, ref in rule_paths_oracle.reference_pairs(c):
            rule = c["rule_rel"][b, k, : c["rule_len"][b, k]].tolist()
            got_n, walks = rule_paths_oracle.pair(by_rel, b * N + s, rule)
            triples = {tuple((nd[i], int(c["rels"][fc[i]]), nd[i + 1]) for i in range(len(fc))) for nd, fc in walks}
            assert got_n == n == len(walks) and triples == ref, (name, b, s, k, n, got_n)
            assert [w[0] for w in walks] == sorted(w[0] for w in walks), (name, "rank order")
            nonempty += n > 0
        stats[name] = (len(c["ref_pair"]), nonempty, int(c["ref_pair"][:, 3].max()))
    return stats


def time_reference(gu, out, per=4):
    lines = []
    for name in ("C1", "C3", "C2"):
        B = min(per, synth.CONFIGS[name].B)
        cfg, h, r, t, seed_flag, rules = synth_batch(name, B, np.random.default_rng(TIME_SEED), extra_seeds=0)
        h, r, t = (np.asarray(x) for x in (h, r, t))
        t_build = t_search = 0.0
        n_paths = 0
        for b in range(B):
            t0 = time.perf_counter()
            G = question_graph(gu, h, r, t, b, cfg.N)
            t1 = time.perf_counter()
            for s in np.flatnonzero(seed_flag[b]).tolist():
                for rule in rules[b]:
                    n_paths += len(gu.bfs_with_rule(G, str(b * cfg.N + s), [str(x) for x in rule]))
            t2 = time.perf_counter()
            t_build += t1 - t0
            t_search += t2 - t1
        lines.append(json.dumps({"shape": name, "questions": B, "rules_per_question": R_SLOTS, "max_rule_hops": 3,
                                 "paths_per_question": n_paths / B, "search_ms_per_question": 1e3 * t_search / B,
                                 "with_build_graph_ms_per_question": 1e3 * (t_search + t_build) / B}))
        print(lines[-1], flush=True)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("GNNRAG_REFERENCE"),
                    help="checkout of the reference (cmavro/GNN-RAG); default: $GNNRAG_REFERENCE")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--time-out", default=None, help="with --time: also write the lines to this file")
    ap.add_argument("--out", default=os.path.join(HERE, "rule_paths_ref.npz"))
    a = ap.parse_args()
    if not a.reference:
        ap.error("--reference (or GNNRAG_REFERENCE) must name a checkout of the reference")
    gu = load_reference(a.reference)
    if a.time:
        time_reference(gu, a.time_out)
        return
    cases = make_cases(gu)
    stats = check_against_oracle(cases)
    flat = {"%s/%s" % (n, k): v for n, c in cases.items() for k, v in c.items()}
    np.savez_compressed(a.out, **flat)
    print("wrote", a.out, os.path.getsize(a.out), "bytes; (pairs, non-empty, largest count):", stats)


if __name__ == "__main__":
    main()
