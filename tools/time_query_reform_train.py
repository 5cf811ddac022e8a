#!/usr/bin/env python
"""The instruction update between two ReaRev iterations under autograd with ``GNNRAG_HIP_QUERY_REFORM_TRAIN`` off (the
reference's ``torch.bmm`` + ``Fusion`` and autograd's backward of them) and on (``autograd.QueryReformFn``:
``gnnrag_query_reform_train`` / ``gnnrag_query_reform_backward``, the reforms of an iteration in one call), each setting in a
process of its own under its own time limit:

    python tools/time_query_reform_train.py [--iters 20] [--warm 5] [--out profiles/query_reform_train_time.jsonl]

* the module sequence: a stand-in with n bound ``QueryReform`` modules (tests/query_reform_grad_oracle.py) and a LEAF node
  state runs one iteration's reforms (rearev.py:217-221) and one backward of a loss over every output; shapes (B, N, D, n) =
  (16, 2000, 200, 2) and (64, 2000, 200, 2).  HIP events around each forward + backward, median of ``--iters`` after
  ``--warm``, min and max beside it.
* the node-state pass alone (``k_qr_dent``, the one memory-bound kernel; switch-on process only): ten backward calls that
  want ``d_ent`` alone between two events, minus ten that want ``dq`` alone (both run ``k_qr_bwd`` with the transposed
  products; only the first runs the pass), per call; achieved bytes/s = B N D 4 bytes over that time, beside the box's copy
  ceiling.  A difference of two event times: an estimate, not a profile.

One JSON line per measurement, printed and appended to ``--out``."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(16, 2000, 200, 2), (64, 2000, 200, 2)]
TAG = "GNNRAG_QR_TRAIN "
CHILD_LIMIT_S = 300
COPY_CEILING_TBS = 5.81
REPEAT = 10


def _median(xs):
    xs = sorted(xs)
    n = len(xs)
    return xs[n // 2] if n % 2 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])


def _timed(torch, fn, n, warm):
    """fn(it) n times; HIP-event ms of the iterations after ``warm``."""
    ms = []
    for it in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn(it)
        e1.record()
        e1.synchronize()
        if it >= warm:
            ms.append(e0.elapsed_time(e1))
    return ms


def child(a):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import torch
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import ops
    from gnnrag_amd.modules.query_update import bind_reforms, train_enabled
    import query_reform_grad_oracle as qo
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_query_reform_train.py needs a GPU")
    dev = torch.device("cuda", 0)
    calls = {"n": 0}
    inner = ops.query_reform_train

    def counted(*args, **kw):
        calls["n"] += 1
        return inner(*args, **kw)

    ops.query_reform_train = counted
    for B, N, D, n in SHAPES:
        torch.manual_seed(B + D)
        c = qo.train_case(B, N, D, n, seed=B)
        model = bind_reforms(qo.standin(D, n).to(dev).train())
        ins0 = [torch.from_numpy(q).to(dev).requires_grad_(True) for q in c["qs"]]
        ent = torch.from_numpy(c["ent"]).to(dev).requires_grad_(True)
        seed, mask = torch.from_numpy(c["seed"]).to(dev), torch.ones(B, N, device=dev)
        losses = []

        def sequence(it):
            model.zero_grad(set_to_none=True)
            ent.grad = None
            for t in ins0:
                t.grad = None
            outs = model.loop(ins0, [ent], seed, mask)
            loss = sum((o * o).sum() for o in outs)
            loss.backward()
            losses.append(loss.detach())

        calls["n"] = 0
        ms = _timed(torch, sequence, a.warm + a.iters, a.warm)
        rec = {"what": "module_sequence_fwd_bwd", "switch": "on" if train_enabled() else "off", "B": B, "N": N, "D": D, "n": n,
               "event_ms": _median(ms), "event_ms_min": min(ms), "event_ms_max": max(ms), "iters": a.iters, "warm": a.warm,
               "query_reform_train_calls_per_iteration": calls["n"] / (a.warm + a.iters), "loss_last": float(losses[-1]),
               "ent_grad_checksum": float(ent.grad.double().abs().sum()),
               "weight_grad_checksum": float(model.reform0.fusion.r.weight.grad.double().abs().sum()),
               "device": torch.cuda.get_device_name(0)}
        print(TAG + json.dumps(rec), flush=True)
        if not train_enabled():
            continue
        t = {k: ([torch.from_numpy(x).to(dev) for x in v] if isinstance(v, list) else torch.from_numpy(v).to(dev))
             for k, v in c.items()}
        _, reserve = inner(t["qs"], t["seed"], t["ent"], t["W_rs"], t["W_gs"])
        G = list(t["G"].unbind(0))

        def bwd(need):
            def run(it):
                for _ in range(REPEAT):
                    ops.query_reform_backward(t["qs"], t["seed"], t["W_rs"], t["W_gs"], reserve, G, need=need)
            return run

        with_pass = _median(_timed(torch, bwd({"d_ent": True}), a.warm + a.iters, a.warm)) / REPEAT
        without = _median(_timed(torch, bwd({"dq": True}), a.warm + a.iters, a.warm)) / REPEAT
        ms_pass = with_pass - without
        nbytes = B * N * D * 4
        rec = {"what": "k_qr_dent_by_difference", "B": B, "N": N, "D": D, "n": n, "bytes_written": nbytes,
               "backward_d_ent_only_ms": with_pass, "backward_dq_only_ms": without, "k_qr_dent_ms": ms_pass,
               "achieved_TBps": (nbytes / (ms_pass * 1e-3) / 1e12) if ms_pass > 0 else None,
               "copy_ceiling_TBps": COPY_CEILING_TBS, "calls_per_event_pair": REPEAT, "iters": a.iters, "warm": a.warm,
               "device": torch.cuda.get_device_name(0)}
        print(TAG + json.dumps(rec), flush=True)


def _spawn(argv, env_extra, lines):
    env = dict(os.environ)
    env.update(env_extra)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, env=env, capture_output=True, text=True,
                           timeout=CHILD_LIMIT_S)
    except subprocess.TimeoutExpired:
        raise SystemExit("child %s ran into its time limit of %d s" % (argv, CHILD_LIMIT_S))
    got = [json.loads(l[len(TAG):]) for l in r.stdout.splitlines() if l.startswith(TAG)]
    if r.returncode != 0:
        raise SystemExit("child %s failed (%d):\n%s" % (argv, r.returncode, (r.stdout + r.stderr)[-3000:]))
    for rec in got:
        print(json.dumps(rec), flush=True)
    lines.extend(got)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "query_reform_train_time.jsonl"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    common = ["--child", "--iters", str(a.iters), "--warm", str(a.warm)]
    lines = []
    # a failing child ends the run: nothing more is started on the device after it
    for switch in ("0", "1"):
        _spawn(common, {"GNNRAG_HIP_QUERY_REFORM_TRAIN": switch}, lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
