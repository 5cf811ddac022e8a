"""Plain-Python restatement of the reasoning-path contract (test infrastructure, no GPU, no networkx).

Graph of a question: facts with head != tail; the facts joining one unordered pair of nodes are one edge, its winning
fact the one with the largest fact id.  Paths of a pair: all shortest paths seed .. candidate, ranked lexicographically by
their node sequence read from the candidate back to the seed.  ``tests/golden/paths_ref.npz`` (written from the live
reference by ``tests/golden/make_golden_paths.py``) pins this restatement to ``build_graph`` + ``get_truth_paths``."""
import os

import numpy as np

INT32_MAX = 2 ** 31 - 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "paths_ref.npz")


def adjacency(heads, tails):
    """node -> ascending list of (neighbour, winning fact id)."""
    win = {}
    for f, (a, b) in enumerate(zip(heads, tails)):
        if a != b:
            win[(a, b) if a < b else (b, a)] = f          # later facts overwrite: the largest fact id wins
    adj = {}
    for (a, b), f in win.items():
        adj.setdefault(a, []).append((b, f))
        adj.setdefault(b, []).append((a, f))
    for v in adj:
        adj[v].sort()
    return adj


def ugraph_numpy(heads, tails, BN):
    """(u_ptr [BN+1], u_adj [U,2]) as gnnrag_ugraph_build lays them out."""
    adj = adjacency(np.asarray(heads).tolist(), np.asarray(tails).tolist())
    u_ptr = np.zeros(BN + 1, dtype=np.int32)
    rows = []
    for v in range(BN):
        row = adj.get(v, [])
        u_ptr[v + 1] = u_ptr[v] + len(row)
        rows.extend(row)
    return u_ptr, np.asarray(rows, dtype=np.int32).reshape(-1, 2)


def levels(adj, s, max_hops=None):
    """Level and number of shortest paths from s of every node within max_hops."""
    lev, sig = {s: 0}, {s: 1}
    frontier, l = [s], 0
    while frontier and (max_hops is None or l < max_hops):
        l += 1
        nxt = {}
        for u in frontier:
            for v, _ in adj.get(u, ()):
                if v not in lev:
                    nxt[v] = nxt.get(v, 0) + sig[u]
        for v, k in nxt.items():
            lev[v], sig[v] = l, k
        frontier = list(nxt)
    return lev, sig


def ranked_paths(adj, lev, s, c, limit=None):
    """Paths s .. c as (nodes from s to c, winning facts) in rank order, at most ``limit``."""
    out = []

    def rec(v, nodes, facts):
        if limit is not None and len(out) >= limit:
            return
        if v == s:
            out.append((tuple(reversed(nodes)), tuple(reversed(facts))))
            return
        for u, f in adj[v]:
            if lev.get(u, -9) == lev[v] - 1:
                rec(u, nodes + [u], facts + [f])

    rec(c, [c], [])
    return out


def pair(adj, s, c, max_paths=None, max_hops=None, lev_sig=None):
    """(n_paths, hops, paths) of one pair; (0, -1, []) when there is no path."""
    if s not in adj or c not in adj:
        return 0, -1, []
    lev, sig = lev_sig if lev_sig is not None else levels(adj, s, max_hops)
    if c not in lev:
        return 0, -1, []
    return min(sig[c], INT32_MAX), lev[c], ranked_paths(adj, lev, s, c, max_paths)


def batch(heads, tails, B, N, seed_flag, cand_slot, cand_cnt, max_seeds, max_cands, max_paths, max_hops):
    """What gnnrag_shortest_paths returns: q_info [B,2], pair_info [B,S,C,2], and per pair index the list of
    (nodes, facts) records in rank order."""
    adj = adjacency(np.asarray(heads).tolist(), np.asarray(tails).tolist())
    S, C = max_seeds, max_cands
    q_info = np.zeros((B, 2), dtype=np.int32)
    pair_info = np.zeros((B, S, C, 2), dtype=np.int32)
    pair_info[..., 1] = -1
    records = {}
    for b in range(B):
        seeds = np.flatnonzero(np.asarray(seed_flag[b]) != 0)
        q_info[b] = (len(seeds), max(int(cand_cnt[b][1]), 0))
        nc = min(int(q_info[b, 1]), C, N)
        for si, s in enumerate(seeds[:S].tolist()):
            ls = levels(adj, b * N + s, max_hops)
            for ci in range(nc):
                c = int(cand_slot[b][ci])
                if c < 0 or c >= N:
                    continue
                n, h, ps = pair(adj, b * N + s, b * N + c, max_paths, max_hops, ls)
                pair_info[b, si, ci] = (n, h)
                records[(b * S + si) * C + ci] = ps
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
    """The fixture's reference result per pair: [(b, seed slot, cand slot, n_paths, set of triple tuples)], in the order
    of get_truth_paths' loops."""
    rp, owner, tri = case["ref_pair"], case["ref_path_pair"], case["ref_paths"]
    sets = [set() for _ in range(len(rp))]
    for i, p in enumerate(owner.tolist()):
        row = tri[i]
        sets[p].add(tuple(tuple(int(x) for x in t) for t in row if t[0] >= 0))
    return [(int(b), int(s), int(c), int(n), sets[i]) for i, (b, s, c, n) in enumerate(rp.tolist())]


def as_triples(records, rels):
    """{(nodes, facts)} -> set of ((u, relation, v), ...) in path direction."""
    return {tuple((nd[i], int(rels[fc[i]]), nd[i + 1]) for i in range(len(fc))) for nd, fc in records}


def device_records(path_off, path_nodes, path_facts, p, hops):
    """Records of pair p from the device arrays as [(nodes, facts)] in written order."""
    out = []
    for r in range(int(path_off[p]), int(path_off[p + 1])):
        out.append((tuple(int(x) for x in path_nodes[r, : hops + 1]), tuple(int(x) for x in path_facts[r, :hops])))
    return out
