#!/usr/bin/env python
"""Device time of the reasoning-path retrieval on the synthetic shapes: the adjacency build (gnnrag_ugraph_build), the
path call (gnnrag_shortest_paths: levels + counts, offsets, unranking) and retrieve_paths end to end (selection, paths,
readback, Python records), per batch.  HIP events around each stage, warm-up, median of the repetitions; one JSON line
per shape.  The reference's own time for the same search is reported by tests/golden/make_golden_paths.py --time (on
the CPU it runs on).

    python tools/time_paths.py [--shapes C1,C3,C2,C4] [--reps 20] [--out FILE]

``--rules`` measures the rule-guided walks instead (gnnrag_rule_paths alone, and retrieve_rule_paths with its readback and
Python records) on C1 / C3 / C2 with 8 sampled rules of 1 - 3 hops per question, and appends one line per shape to
``--rules-out`` (default profiles/rule_paths_time.jsonl); the reference's time for the same rules on the same graphs
comes from tests/golden/make_golden_rule_paths.py --time.

    python tools/time_paths.py --rules [--shapes C1,C3,C2] [--reps 20] [--rules-out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gnnrag_amd  # noqa: E402,F401
from gnnrag_amd import ops, paths, synth  # noqa: E402


def peaked_pred(rng, batch):
    """A few eligible slots share 0.97 of the mass (a trained model's answer distribution is peaked): the top-p cut
    retrieves a handful of candidates per question."""
    B, N = batch.local_entity.shape
    p = np.zeros((B, N), dtype=np.float64)
    for b in range(B):
        n = int(batch.n_real[b])
        if n < 2:
            continue
        top = rng.choice(np.arange(1, n), min(int(rng.integers(3, 11)), n - 1), replace=False)
        p[b, :n] = 0.03 * rng.dirichlet(np.ones(n))
        p[b, top] += 0.97 * rng.dirichlet(np.ones(len(top)) * 4.0)
    return p.astype(np.float32)


def events_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def run(shape, reps, limits, batch_seed=None):
    cfg = synth.CONFIGS[shape]
    batch = synth.make_batch(cfg, seed=batch_seed)
    h, r, t = batch.edge_tuple[:3]
    dev = torch.device("cuda", 0)
    plan = ops.CsrPlan(h, r, t, cfg.B, cfg.N, cfg.R1, dev)
    S, C, K, H = limits
    pred = torch.from_numpy(peaked_pred(np.random.default_rng(1234), batch)).to(dev)
    seeds = batch.query_entities == 1
    el = torch.from_numpy(((~seeds) & (batch.local_entity != batch.num_entity)).astype(np.uint8)).to(dev)
    sf = torch.from_numpy(seeds.astype(np.uint8)).to(dev)
    eps = 0.95
    ignore = (1 - eps) / cfg.N
    build = events_ms(lambda: ops.UGraph.from_plan(plan), reps)
    graph = ops.UGraph.from_plan(plan)
    slots, cnt = ops.topp_candidates(pred, el, ignore, eps)
    buf = ops.PathBuffers(cfg.B, cfg.N, S, C, K, H, dev)
    call = events_ms(lambda: ops.shortest_paths(graph, sf, slots, cnt, S, C, K, H, buffers=buf), reps)
    select = events_ms(lambda: ops.topp_candidates(pred, el, ignore, eps), reps)

    def readback():
        off = buf.path_off.cpu()
        n = int(off[-1])
        buf.q_info.cpu(), buf.pair_info.cpu(), buf.path_nodes[:n].cpu(), buf.path_facts[:n].cpu()

    rb = events_ms(readback, reps)
    walls = []
    for i in range(reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = paths.retrieve_paths(graph, r, pred, batch.local_entity, batch.query_entities, batch.num_entity, ignore, eps,
                                   S, C, K, H)
        if i >= 2:
            walls.append(1e3 * (time.perf_counter() - t0))
    pairs = [p for q in res for p in q]
    return {"shape": shape, "batch_seed": cfg.seed if batch_seed is None else batch_seed, "B": cfg.B, "N": cfg.N, "facts": int(len(h)), "limits": dict(max_seeds=S, max_cands=C, max_paths=K, max_hops=H),
            "adjacency_records": int(graph.to_host()["u_ptr"][-1]),
            "ugraph_build_ms": build[0], "ugraph_build_min_max_ms": build[1:],
            "select_ms": select[0], "shortest_paths_ms": call[0], "shortest_paths_min_max_ms": call[1:],
            "readback_ms": rb[0], "retrieve_paths_wall_ms": float(np.median(walls)),
            "retrieve_paths_wall_ms_per_question": float(np.median(walls)) / cfg.B,
            "pairs": len(pairs), "pairs_with_paths": sum(p["n_paths"] > 0 for p in pairs),
            "paths_written": sum(len(p["paths"]) for p in pairs), "max_n_paths": max([p["n_paths"] for p in pairs] + [0]),
            "max_hops_seen": max([p["hops"] for p in pairs] + [-1]),
            "share_of_pairs_cut": float(np.mean([p["n_paths"] > K for p in pairs])) if pairs else 0.0,
            "readback_bytes": dict(paths.LAST_READBACK), "reps": reps, "device": torch.cuda.get_device_name(0)}


RULE_SEED = 1234            # tests/golden/make_golden_rule_paths.py --time samples the same rules (TIME_SEED)


def run_rules(shape, reps, limits):
    cfg = synth.CONFIGS[shape]
    batch = synth.make_batch(cfg)
    h, r, t = batch.edge_tuple[:3]
    dev = torch.device("cuda", 0)
    S, R, K, H = limits
    seeds = batch.query_entities == 1
    rules = synth.sample_rules(h, r, t, cfg.B, cfg.N, seeds, R, 3, np.random.default_rng(RULE_SEED), n_rel=cfg.R)
    rule_rel, rule_len = paths._pack_rules(rules, cfg.B, None, R, H)
    graph = ops.UGraph.from_plan(ops.CsrPlan(h, r, t, cfg.B, cfg.N, cfg.R1, dev))
    fr = torch.from_numpy(np.asarray(r, dtype=np.int32)).to(dev)
    sf = torch.from_numpy(seeds.astype(np.uint8)).to(dev)
    rr, rl = torch.from_numpy(rule_rel).to(dev), torch.from_numpy(rule_len).to(dev)
    buf = ops.RulePathBuffers(graph.F, cfg.B, cfg.N, S, R, K, H, dev)
    call = events_ms(lambda: ops.rule_paths(graph, fr, sf, rr, rl, S, R, K, H, buffers=buf), reps)
    walls = []
    for i in range(reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = paths.retrieve_rule_paths(graph, r, batch.local_entity, batch.query_entities, rules, None, S, R, K, H)
        if i >= 2:
            walls.append(1e3 * (time.perf_counter() - t0))
    pairs = [p for q in res for p in q]
    return {"shape": shape, "batch_seed": cfg.seed, "rule_seed": RULE_SEED, "B": cfg.B, "N": cfg.N, "facts": int(len(h)),
            "limits": dict(max_seeds=S, max_rules=R, max_paths=K, max_hops=H),
            "workspace_bytes": int(buf.ws.numel()), "count_workgroups": cfg.B * R,
            "rule_paths_ms": call[0], "rule_paths_min_max_ms": call[1:],
            "retrieve_rule_paths_wall_ms": float(np.median(walls)),
            "retrieve_rule_paths_wall_ms_per_question": float(np.median(walls)) / cfg.B,
            "pairs": len(pairs), "pairs_with_paths": sum(p["n_paths"] > 0 for p in pairs),
            "paths_written": sum(len(p["paths"]) for p in pairs), "max_n_paths": max([p["n_paths"] for p in pairs] + [0]),
            "share_of_pairs_cut": float(np.mean([p["n_paths"] > K for p in pairs])) if pairs else 0.0,
            "readback_bytes": dict(paths.LAST_RULE_READBACK), "reps": reps, "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C1,C3,C2,C4")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limits", default="4,16,64,8", help="max_seeds,max_cands,max_paths,max_hops")
    ap.add_argument("--batch-seed", type=int, default=None, help="seed of the synthetic batch (default: the shape's own)")
    ap.add_argument("--rules", action="store_true", help="measure the rule-guided walks instead (C1,C3,C2 by default)")
    ap.add_argument("--rule-limits", default="4,8,64,4", help="with --rules: max_seeds,max_rules,max_paths,max_hops")
    ap.add_argument("--rules-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                        "profiles", "rule_paths_time.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_paths.py measures on the GPU; none is visible")
    if a.rules:
        shapes = "C1,C3,C2" if a.shapes == ap.get_default("shapes") else a.shapes
        os.makedirs(os.path.dirname(os.path.abspath(a.rules_out)), exist_ok=True)
        for shape in shapes.split(","):
            line = json.dumps(run_rules(shape, a.reps, tuple(int(x) for x in a.rule_limits.split(","))))
            print(line, flush=True)
            with open(a.rules_out, "a") as f:
                f.write(line + "\n")
        return
    limits = tuple(int(x) for x in a.limits.split(","))
    lines = []
    for shape in a.shapes.split(","):
        rec = run(shape, a.reps, limits, a.batch_seed)
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
