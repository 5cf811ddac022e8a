"""Reasoning paths: the retrieval output of GNN-RAG, on the device.

After the GNN has scored a question's subgraph, the reference joins every question entity to every retrieved candidate
by all shortest paths of the subgraph and hands those paths - not the probabilities - to the LLM
(``llm/src/utils/graph_utils.py``: ``build_graph`` + ``get_truth_paths``, called from
``llm/src/qa_prediction/build_qa_input.py:114-127``).  That is a networkx graph per question and one
``nx.all_shortest_paths`` per pair.  :func:`retrieve_paths` does it with the structure that is already on the GPU: the
candidate selection of the Evaluator (``gnnrag_topp_candidates``), the levels / path counts and the path records are
enqueued on one stream, and ONE synchronising readback brings back the paths that exist.

    from gnnrag_amd.paths import retrieve_paths, path_to_string
    per_question = retrieve_paths(plan, rels, pred_dist, local_entity, query_entities, pad_ent_id, ignore_prob, eps)
    for pair in per_question[0]:
        for path in pair["paths"]:
            print(path_to_string(path))

The reference's other path set, the walks that follow a predicted relation path ("rule") from a question entity
(``bfs_with_rule``, called by ``apply_rules`` of ``build_qa_input.py``), comes from :func:`retrieve_rule_paths` on the
same adjacency, and :func:`reasoning_context` joins the two the way ``PromptBuilder.process_input`` does (GNN-RAG+RA).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops

# what the last retrieve_paths call copied back (tests assert the readback is O(paths written)): bytes of the two
# small fixed blocks and of the record prefix, and the number of records
LAST_READBACK = {"fixed_bytes": 0, "record_bytes": 0, "records": 0}
# the same for the last retrieve_rule_paths call
LAST_RULE_READBACK = {"fixed_bytes": 0, "record_bytes": 0, "records": 0}


def path_to_string(path) -> str:
    """``"h -> r -> t -> r -> t"`` for a path ``[(h, r, t), (t, r, t'), ...]`` - the rendering the reference gives the
    LLM (``llm/src/utils/utils.py:34-44``): the first triple's head, then relation and tail of every triple."""
    out = []
    for i, (h, r, t) in enumerate(path):
        if i == 0:
            out.append(str(h))
        out.append(str(r))
        out.append(str(t))
    return " -> ".join(out)


def _name(mapping, i):
    if mapping is None:
        return i
    return mapping[i]


def retrieve_paths(plan_or_ugraph, rels, pred_dist: torch.Tensor, local_entity, query_entities, pad_ent_id: int,
                   ignore_prob: float, eps: float, max_seeds: int = 4, max_cands: int = 16, max_paths: int = 64,
                   max_hops: int = 8, id2entity=None, id2relation=None, return_info: bool = False):
    """Per question the list ``[{"seed", "cand", "n_paths", "hops", "paths": [[(u, rel, v), ...], ...]}, ...]`` over its
    (question entity, retrieved candidate) pairs, seeds outermost, candidates best first - the loops of
    ``get_truth_paths``.  Entities are global ids through ``local_entity`` (names through ``id2entity`` /
    ``id2relation`` when given), every triple in path direction.

    ``plan_or_ugraph``: the batch's :class:`ops.CsrPlan` (its adjacency is derived here) or an :class:`ops.UGraph` made
    from it (keep it with a cached batch).  ``rels``: the relation id of every fact of the batch tuple (its second
    array).  ``pred_dist`` [B, N] stays on the GPU; the candidates are those of ``eval_tail.retrieved_candidates`` (same
    eligibility rule, same kernel).  ``n_paths`` is the true number of shortest paths; ``len(paths) == min(n_paths,
    max_paths)``; ``hops == -1``: not reached within ``max_hops``.  ``return_info=True`` returns ``(result, info)`` with
    ``info[b] = (seeds found, candidates retrieved)``: values above ``max_seeds`` / ``max_cands`` say the question was
    cut."""
    if not isinstance(pred_dist, torch.Tensor) or not pred_dist.is_cuda:
        raise _lib.GnnragError("pred_dist must live on the GPU; there is no CPU path")
    graph = plan_or_ugraph if isinstance(plan_or_ugraph, ops.UGraph) else ops.UGraph.from_plan(plan_or_ugraph)
    dev = graph.device
    B, N = graph.B, graph.N
    local_entity = np.asarray(local_entity)
    qe = np.asarray(query_entities)
    if local_entity.shape != (B, N) or qe.shape != (B, N) or tuple(pred_dist.shape) != (B, N):
        raise ValueError("local_entity, query_entities and pred_dist must be [%d, %d]" % (B, N))
    rels = np.asarray(rels)
    seeds = qe.astype(np.int64) == 1                                   # evaluate.py:177
    eligible = (~seeds) & (local_entity != pad_ent_id)                 # evaluate.py:198-205
    with torch.cuda.device(dev):
        el = torch.from_numpy(eligible.astype(np.uint8)).to(dev)
        sf = torch.from_numpy(seeds.astype(np.uint8)).to(dev)
        slots, cnt = ops.topp_candidates(pred_dist.detach().float().contiguous(), el, ignore_prob, eps)
        out = ops.shortest_paths(graph, sf, slots, cnt, max_seeds, max_cands, max_paths, max_hops)
        # the one synchronising readback: the small fixed blocks, then the records that exist
        fixed = torch.cat([out.q_info.reshape(-1), out.pair_info.reshape(-1), out.path_off,
                           slots[:, :max_cands].reshape(-1)]).cpu().numpy()
        P = B * max_seeds * max_cands
        q_info = fixed[: 2 * B].reshape(B, 2)
        pair_info = fixed[2 * B: 2 * B + 2 * P].reshape(B, max_seeds, max_cands, 2)
        path_off = fixed[2 * B + 2 * P: 2 * B + 3 * P + 1]
        slots_h = fixed[2 * B + 3 * P + 1:].reshape(B, -1)
        total = int(path_off[-1])
        nodes = out.path_nodes[:total].cpu().numpy()
        facts = out.path_facts[:total].cpu().numpy()
    LAST_READBACK.update(fixed_bytes=int(fixed.nbytes), record_bytes=int(nodes.nbytes + facts.nbytes),
                         records=total)
    result = []
    for b in range(B):
        seed_slots = np.flatnonzero(seeds[b])[:max_seeds]
        n_c = min(int(q_info[b, 1]), max_cands)
        pairs = []
        for si, s in enumerate(seed_slots):
            for ci in range(n_c):
                c = int(slots_h[b, ci])
                p = (b * max_seeds + si) * max_cands + ci
                paths = []
                h = int(pair_info[b, si, ci, 1])
                for r in range(int(path_off[p]), int(path_off[p + 1])):
                    ent = [_name(id2entity, int(local_entity[b, v - b * N])) for v in nodes[r, : h + 1]]
                    paths.append([(ent[i], _name(id2relation, int(rels[facts[r, i]])), ent[i + 1]) for i in range(h)])
                pairs.append({"seed": _name(id2entity, int(local_entity[b, s])),
                              "cand": _name(id2entity, int(local_entity[b, c])),
                              "seed_slot": int(s), "cand_slot": c,
                              "n_paths": int(pair_info[b, si, ci, 0]), "hops": h, "paths": paths})
        result.append(pairs)
    return (result, q_info.copy()) if return_info else result


def _pack_rules(rules, B, relation2id, max_rules, max_hops):
    """rules[b] = list of relation-id lists (or name lists through ``relation2id``) -> (rule_rel [B,R,H], rule_len [B,R])."""
    if len(rules) != B:
        raise ValueError("rules must hold one list per question (%d), got %d" % (B, len(rules)))
    rule_rel = np.full((B, max_rules, max_hops), -1, dtype=np.int32)
    rule_len = np.zeros((B, max_rules), dtype=np.int32)
    for b, rs in enumerate(rules):
        if len(rs) > max_rules:
            raise ValueError("question %d has %d rules, max_rules is %d" % (b, len(rs), max_rules))
        for k, rule in enumerate(rs):
            if len(rule) > max_hops:
                raise ValueError("rule %d of question %d has %d hops, max_hops is %d" % (k, b, len(rule), max_hops))
            ids = [int(relation2id.get(x, -1)) if relation2id is not None else int(x) for x in rule]
            rule_rel[b, k, : len(ids)] = ids
            rule_len[b, k] = len(ids)
    return rule_rel, rule_len


def retrieve_rule_paths(plan_or_ugraph, rels, local_entity, query_entities, rules, relation2id=None, max_seeds: int = 4,
                        max_rules: int = 8, max_paths: int = 64, max_hops: int = 4, id2entity=None, id2relation=None,
                        return_info: bool = False):
    """Per question the list ``[{"seed", "seed_slot", "rule", "n_paths", "hops", "paths": [[(u, rel, v), ...], ...]},
    ...]`` over its (question entity, rule) pairs, seeds outermost, rules in the given order - the loops of
    ``apply_rules``.  A path is a walk from the seed whose hop ``i`` is an edge of relation ``rule[i]`` (nodes may
    repeat), every triple in walk direction, in ascending order of the walk's node sequence.

    ``rules[b]``: the question's rules, each a list of relation ids, or of relation names mapped through ``relation2id``
    (an unknown name becomes -1 and matches nothing, as an unknown string does in the reference).  More than
    ``max_rules`` rules or a rule longer than ``max_hops`` raise ``ValueError``; an empty rule yields ``n_paths == 0``
    (the reference's single empty path carries no triple).  ``n_paths`` is the true number of walks;
    ``len(paths) == min(n_paths, max_paths)``.  The other arguments and ``return_info`` are those of
    :func:`retrieve_paths`; ``info[b] = (seeds found, rules of 1 .. max_hops hops)``."""
    B, N = plan_or_ugraph.B, plan_or_ugraph.N
    rule_rel, rule_len = _pack_rules(rules, B, relation2id, max_rules, max_hops)      # raises before any device work
    graph = plan_or_ugraph if isinstance(plan_or_ugraph, ops.UGraph) else ops.UGraph.from_plan(plan_or_ugraph)
    dev = graph.device
    local_entity = np.asarray(local_entity)
    qe = np.asarray(query_entities)
    if local_entity.shape != (B, N) or qe.shape != (B, N):
        raise ValueError("local_entity and query_entities must be [%d, %d]" % (B, N))
    rels = np.asarray(rels)
    seeds = qe.astype(np.int64) == 1
    with torch.cuda.device(dev):
        sf = torch.from_numpy(seeds.astype(np.uint8)).to(dev)
        fr = torch.from_numpy(np.ascontiguousarray(rels, dtype=np.int32)).to(dev)
        out = ops.rule_paths(graph, fr, sf, torch.from_numpy(rule_rel).to(dev), torch.from_numpy(rule_len).to(dev),
                             max_seeds, max_rules, max_paths, max_hops)
        # the one synchronising readback: the small fixed blocks, then the records that exist
        fixed = torch.cat([out.q_info.reshape(-1), out.pair_info.reshape(-1), out.path_off]).cpu().numpy()
        P = B * max_seeds * max_rules
        q_info = fixed[: 2 * B].reshape(B, 2)
        pair_info = fixed[2 * B: 2 * B + 2 * P].reshape(B, max_seeds, max_rules, 2)
        path_off = fixed[2 * B + 2 * P:]
        total = int(path_off[-1])
        nodes = out.path_nodes[:total].cpu().numpy()
        facts = out.path_facts[:total].cpu().numpy()
    LAST_RULE_READBACK.update(fixed_bytes=int(fixed.nbytes), record_bytes=int(nodes.nbytes + facts.nbytes),
                              records=total)
    result = []
    for b in range(B):
        pairs = []
        for si, s in enumerate(np.flatnonzero(seeds[b])[:max_seeds]):
            for k, rule in enumerate(rules[b]):
                p = (b * max_seeds + si) * max_rules + k
                h = int(pair_info[b, si, k, 1])
                paths = []
                for r in range(int(path_off[p]), int(path_off[p + 1])):
                    ent = [_name(id2entity, int(local_entity[b, v - b * N])) for v in nodes[r, : h + 1]]
                    paths.append([(ent[i], _name(id2relation, int(rels[facts[r, i]])), ent[i + 1]) for i in range(h)])
                pairs.append({"seed": _name(id2entity, int(local_entity[b, s])), "seed_slot": int(s), "rule": list(rule),
                              "n_paths": int(pair_info[b, si, k, 0]), "hops": h, "paths": paths})
        result.append(pairs)
    return (result, q_info.copy()) if return_info else result


def reasoning_context(rule_result_b, shortest_result_b):
    """The ordered list of path strings of one question as ``PromptBuilder.process_input`` assembles it
    (``llm/src/qa_prediction/build_qa_input.py:105-123``, the GNN-RAG+RA union): every rule path in result order, then
    each shortest path whose string is not in the list yet.  ``rule_result_b`` / ``shortest_result_b``: one question's
    entry of :func:`retrieve_rule_paths` / :func:`retrieve_paths` (either may be ``None`` or empty).  Host code."""
    out = [path_to_string(p) for pair in (rule_result_b or ()) for p in pair["paths"]]
    for pair in (shortest_result_b or ()):
        for p in pair["paths"]:
            s = path_to_string(p)
            if s not in out:
                out.append(s)
    return out
