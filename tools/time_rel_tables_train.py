#!/usr/bin/env python
"""The per-question relation tables of the fused training form (``ReasonGNNLayer._forward_autograd`` without active dropout)
with ``GNNRAG_HIP_REL_TABLES_TRAIN`` off (``autograd.relation_tables_dense``: two index_selects, a product, a relu, a slice
stack and an einsum per direction, and autograd's backward of them) and on (``autograd.RelationTablesFn``:
``gnnrag_relation_tables`` / ``gnnrag_relation_tables_backward``), each setting in a process of its own under its own time
limit:

    python tools/time_rel_tables_train.py [--iters 20] [--warm 5] [--ref oracle/_ref/gnn] [--step-runs 2]
                                          [--out profiles/rel_tables_train_time.jsonl]

* the tables alone: LEAF T_fwd, T_inv [R1, D], ins [B, I, D] and W [D, (2I+1) D] on the structure of a ``synth`` batch; one
  forward and one backward of a loss over P; (B, N, D, I) = (16, 2000, 200, 2) and (64, 2000, 200, 2) (the C2 workload's
  edges and relations).  Per iteration the stream time (HIP events around forward + backward) and the host time (a host
  clock from the first call to the return of ``backward()``, before any wait for the device: what the host spends
  enqueueing); median of ``--iters`` after ``--warm``, min and max beside it.
* the staged d200 trainer's step (``tools/time_train_step.py``) with the dropouts off (``--linear_dropout 0 --lm_dropout 0``:
  the layer then takes the fused form), 20 steps after 5, ``--step-runs`` runs per setting, the settings alternating; skipped
  when ``--ref`` does not exist.

Switch off is the code path of the commit before the switch existed and is the baseline.  One JSON line per measurement,
printed and appended to ``--out``."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(16, 2000, 200, 2), (64, 2000, 200, 2)]
TAG = "GNNRAG_RT_TRAIN "
CHILD_LIMIT_S = 300
STEP_LIMIT_S = 420
SWITCH = "GNNRAG_HIP_REL_TABLES_TRAIN"


def _median(xs):
    xs = sorted(xs)
    n = len(xs)
    return xs[n // 2] if n % 2 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])


def child(a):
    sys.path.insert(0, REPO)
    import dataclasses
    import torch
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import ops, synth
    from gnnrag_amd.autograd import RelationTablesFn, relation_tables_dense
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_rel_tables_train.py needs a GPU")
    dev = torch.device("cuda", 0)
    on = os.environ.get(SWITCH, "0") == "1"
    name = torch.cuda.get_device_name(0)
    for B, N, D, I in SHAPES:
        if a.only_batch and B != a.only_batch:
            continue
        cfg = dataclasses.replace(synth.CONFIGS["C2"], B=B, N=N, D=D, I=I)
        et = synth.make_batch(cfg).edge_tuple
        plan = ops.CsrPlan(et[0], et[1], et[2], B, N, cfg.R1, dev)
        torch.manual_seed(B + D)
        leaf = lambda s, *sh: (s * torch.randn(*sh, device=dev)).requires_grad_(True)      # noqa: E731
        T_fwd, T_inv, ins = leaf(0.5, cfg.R1, D), leaf(0.5, cfg.R1, D), leaf(0.5, B, I, D)
        W = leaf(0.05, D, (2 * I + 1) * D)
        G = torch.randn(2, plan.rel_total, D, device=dev)
        leaves = (T_fwd, T_inv, ins, W)
        kept = {}

        def tables():
            if on:          # ReasonGNNLayer._relation_tables
                return RelationTablesFn.apply(plan, T_fwd, T_inv, ins, W)
            return relation_tables_dense(plan, T_fwd, T_inv, ins, W)

        ev_ms, host_ms = [], []
        for it in range(a.warm + a.iters):
            for t in leaves:
                t.grad = None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            loss = (tables() * G).sum()
            loss.backward()
            e1.record()
            t1 = time.perf_counter()
            e1.synchronize()
            kept["loss"] = loss.detach()
            if it >= a.warm:
                ev_ms.append(e0.elapsed_time(e1))
                host_ms.append((t1 - t0) * 1e3)
        rec = {"what": "rel_tables_fwd_bwd", "switch": "on" if on else "off", "B": B, "N": N, "D": D, "I": I,
               "rel_total": plan.rel_total, "R1": cfg.R1,
               "stream_ms": _median(ev_ms), "stream_ms_min": min(ev_ms), "stream_ms_max": max(ev_ms),
               "host_ms": _median(host_ms), "host_ms_min": min(host_ms), "host_ms_max": max(host_ms),
               "iters": a.iters, "warm": a.warm, "loss_last": float(kept["loss"]),
               "T_fwd_grad_checksum": float(T_fwd.grad.double().abs().sum()),
               "ins_grad_checksum": float(ins.grad.double().abs().sum()),
               "weight_grad_checksum": float(W.grad.double().abs().sum()),
               "peak_memory_MB": torch.cuda.max_memory_allocated() / 2 ** 20, "device": name}
        print(TAG + json.dumps(rec), flush=True)
        del T_fwd, T_inv, ins, W, G, leaves, plan
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()


def _spawn(cmd, env_extra, limit, tag):
    env = dict(os.environ)
    env.update(env_extra)
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        raise SystemExit("child %s ran into its time limit of %d s" % (cmd, limit))
    got = [json.loads(l[len(tag):]) for l in r.stdout.splitlines() if l.startswith(tag)]
    if r.returncode != 0 or not got:
        raise SystemExit("child %s failed (%d):\n%s" % (cmd, r.returncode, (r.stdout + r.stderr)[-3000:]))
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rel_tables_train_time.jsonl"))
    ap.add_argument("--ref", default=os.path.join(REPO, "oracle", "_ref", "gnn"))
    ap.add_argument("--step-runs", type=int, default=2)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--only-batch", type=int, default=0, help="with --child: this batch size only (for a profiler run)")
    a = ap.parse_args()
    if a.child:
        return child(a)
    me = [sys.executable, os.path.abspath(__file__), "--child", "--iters", str(a.iters), "--warm", str(a.warm)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def keep(recs):
        with open(a.out, "a") as f:
            for rec in recs:
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + "\n")

    # a failing child ends the run: nothing more is started on the device after it
    for switch in ("0", "1"):
        keep(_spawn(me, {SWITCH: switch}, CHILD_LIMIT_S, TAG))
    if os.path.isdir(a.ref):
        step = [sys.executable, os.path.join(REPO, "tools", "time_train_step.py"), a.ref, "--variant", "d200", "--steps", "20",
                "--warm", "5", "--linear_dropout", "0", "--lm_dropout", "0"]
        for run in range(a.step_runs):
            for switch in ("0", "1"):
                got = _spawn(step, {SWITCH: switch}, STEP_LIMIT_S, "GNNRAG_TRAIN ")
                keep([dict(what="train_step_d200_no_dropout", switch="on" if switch == "1" else "off", run=run, **got[-1])])
    else:
        print("no staged reference at %s: the trainer's step is not measured" % a.ref, flush=True)


if __name__ == "__main__":
    main()
