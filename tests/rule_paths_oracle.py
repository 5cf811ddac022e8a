"""Plain-Python restatement of the rule-walk contract (test infrastructure, no GPU, no networkx).

Graph of a question: ``paths_oracle.adjacency`` (simple, undirected, the winning fact of an edge = its largest fact id);
an edge's relation is that of its winning fact.  Walks of a (seed, rule) pair: every node sequence ``seed = v0 .. vL`` whose
hop ``i`` is an edge of relation ``rule[i]``; nodes may repeat.  Counted by ``down_L = 1``, ``down_l[v] = sum of
down_{l+1}[u]`` over the neighbours ``u`` of ``v`` joined by relation ``rule[l]`` (saturating at INT32_MAX), ranked
lexicographically by node sequence from the seed outwards.  ``tests/golden/rule_paths_ref.npz`` (written from the live
reference by ``tests/golden/make_golden_rule_paths.py``) pins this restatement to ``build_graph`` + ``bfs_with_rule``."""
import os

import numpy as np

import paths_oracle

INT32_MAX = 2 ** 31 - 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rule_paths_ref.npz")


def rel_adjacency(heads, rels, tails):
    """relation -> node -> ascending list of (neighbour, winning fact id) over the edges of that relation."""
    rels = np.asarray(rels).tolist()
    by_rel = {}
    for v, row in paths_oracle.adjacency(np.asarray(heads).tolist(), np.asarray(tails).tolist()).items():
        for u, f in row:                                  # rows are ascending: the per-relation rows stay ascending
            by_rel.setdefault(rels[f], {}).setdefault(v, []).append((u, f))
    return by_rel


def down_counts(by_rel, rule):
    """[down_0 .. down_{L-1}] as dicts node -> count (absent = 0); down_L = 1 everywhere is not stored."""
    L = len(rule)
    down = [None] * L
    for l in range(L - 1, -1, -1):
        cur = {}
        for v, row in by_rel.get(rule[l], {}).items():
            n = len(row) if l == L - 1 else sum(down[l + 1].get(u, 0) for u, _ in row)
            if n:
                cur[v] = min(n, INT32_MAX)
        down[l] = cur
    return down


def ranked_walks(by_rel, down, s, rule, limit=None):
    """Walks from s as (nodes, winning facts) in rank order, at most ``limit``."""
    L = len(rule)
    out = []

    def rec(v, l, nodes, facts):
        if limit is not None and len(out) >= limit:
            return
        if l == L:
            out.append((tuple(nodes), tuple(facts)))
            return
        for u, f in by_rel.get(rule[l], {}).get(v, ()):
            if l == L - 1 or down[l + 1].get(u, 0) > 0:
                rec(u, l + 1, nodes + [u], facts + [f])

    if L and down[0].get(s, 0) > 0:
        rec(s, 0, [s], [])
    return out


def pair(by_rel, s, rule, max_paths=None, down=None):
    """(n_paths, walks in rank order) of one (seed, rule) pair with a rule of at least one hop."""
    down = down_counts(by_rel, rule) if down is None else down
    return down[0].get(s, 0), ranked_walks(by_rel, down, s, rule, max_paths)


def batch(heads, rels, tails, B, N, seed_flag, rule_rel, rule_len, max_seeds, max_rules, max_paths, max_hops):
    """What gnnrag_rule_paths returns: q_info [B,2], pair_info [B,S,R,2], and per pair index the list of (nodes, facts)
    records in rank order."""
    by_rel = rel_adjacency(heads, rels, tails)
    S, R, H = max_seeds, max_rules, max_hops
    q_info = np.zeros((B, 2), dtype=np.int32)
    pair_info = np.zeros((B, S, R, 2), dtype=np.int32)
    pair_info[..., 1] = -1
    records = {}
    for b in range(B):
        seeds = np.flatnonzero(np.asarray(seed_flag[b]) != 0)
        lens = [int(x) for x in np.asarray(rule_len[b])[:R]]
        q_info[b] = (len(seeds), sum(1 <= n <= H for n in lens))
        for k, n in enumerate(lens):
            if not 1 <= n <= H:
                continue
            rule = [int(x) for x in np.asarray(rule_rel[b][k])[:n]]
            down = down_counts(by_rel, rule)
            for si, s in enumerate(seeds[:S].tolist()):
                cnt, walks = pair(by_rel, b * N + s, rule, max_paths, down)
                pair_info[b, si, k] = (cnt, n)
                records[(b * S + si) * R + k] = walks
    return q_info, pair_info, records


def load_cases():
    """name -> dict of the fixture's arrays for that case."""
    z = np.load(GOLDEN)
    cases = {}
    for key in z.files:
        name, field = key.split("/", 1)
        cases.setdefault(name, {})[field] = z[key]
    return cases


def reference_pairs(case):
    """The fixture's reference result per pair: [(b, seed slot, rule index, n_paths, set of triple tuples)], in the order
    of apply_rules' loops (seeds outermost)."""
    rp, owner, tri = case["ref_pair"], case["ref_path_pair"], case["ref_paths"]
    sets = [set() for _ in range(len(rp))]
    for i, p in enumerate(owner.tolist()):
        sets[p].add(tuple(tuple(int(x) for x in t) for t in tri[i] if t[0] >= 0))
    return [(int(b), int(s), int(k), int(n), sets[i]) for i, (b, s, k, n) in enumerate(rp.tolist())]
