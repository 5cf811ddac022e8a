#!/usr/bin/env python
"""The tail of the reasoning layer under autograd (reasongnn.py:163-169: add, relu, dropout, score_func, mask, softmax) with
``GNNRAG_HIP_LAYER_TAIL_TRAIN`` off (the torch ops ``ReasonGNNLayer._forward_autograd`` runs, and autograd's backward of them)
and on (``autograd.LayerTailFn``: ``gnnrag_layer_tail_train`` / ``gnnrag_layer_tail_backward``, the keep flags drawn as the
module draws them), each setting in a process of its own under its own time limit:

    python tools/time_layer_tail_train.py [--iters 20] [--warm 5] [--out profiles/layer_tail_train_time.jsonl]

* the tail alone: LEAF pre-activations pre_a, pre_b [B*N, D], a ``Linear(D, 1)`` score function and a mask with padded
  nodes; one forward and one backward of a loss over ``dist`` and ``h``; shapes (B, N, D) = (16, 2000, 200) and
  (64, 2000, 200), dropout p = 0 and p = 0.2.  HIP events around each forward + backward, median of ``--iters`` after
  ``--warm``, min and max beside it.
* the row kernels (switch-on process only): ten ``ops.layer_tail_train`` calls between two events minus ten
  ``ops.masked_softmax`` calls give ``k_lt_fwd`` per call; ten ``ops.layer_tail_backward`` calls give the backward's three
  launches per call (``k_lt_bwd`` and two small ones, so its rate is a lower bound).  Achieved bytes/s = the bytes the row
  kernel must move (forward: pre_a, pre_b, keep in, h out; backward: h, g_h, keep in, g_pre out) over that time, beside the
  box's copy ceiling.  Differences of event times: an estimate, not a profile.  At batch 16 the
  tensors fit the 256 MB last-level cache: only the batch-64 rate says anything about HBM.

One JSON line per measurement, printed and appended to ``--out``.  For kernel times from a profiler, run one child under it:
``GNNRAG_HIP_LAYER_TAIL_TRAIN=1 rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_layer_tail_train.py --child
--only-batch 64`` (in a run of its own: tracing slows the host)."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(16, 2000, 200), (64, 2000, 200)]
DROPS = [0.0, 0.2]
TAG = "GNNRAG_LT_TRAIN "
CHILD_LIMIT_S = 300
COPY_CEILING_TBS = 5.81
REPEAT = 10
VERY_NEG_NUMBER = -100000000000


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
    import torch
    import torch.nn.functional as F
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import ops
    from gnnrag_amd.autograd import LayerTailFn
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_layer_tail_train.py needs a GPU")
    dev = torch.device("cuda", 0)
    on = os.environ.get("GNNRAG_HIP_LAYER_TAIL_TRAIN", "0") == "1"
    name = torch.cuda.get_device_name(0)
    for B, N, D in SHAPES:
        if a.only_batch and B != a.only_batch:
            continue
        for p in DROPS:
            torch.manual_seed(B + D)
            pre_a = (0.5 * torch.randn(B * N, D, device=dev)).requires_grad_(True)
            pre_b = (0.5 * torch.randn(B * N, D, device=dev)).requires_grad_(True)
            score_func = torch.nn.Linear(D, 1).to(dev)
            linear_drop = torch.nn.Dropout(p=p).train()
            softmax_d1 = torch.nn.Softmax(dim=1)
            mask = (torch.arange(N, device=dev)[None, :] < torch.randint(N // 2, N, (B, 1), device=dev)).float()
            G_h, G_d = torch.randn(B, N, D, device=dev), torch.randn(B, N, device=dev)
            kept = {}

            def tail():
                if on:      # ReasonGNNLayer._layer_tail
                    keep, scale = None, 1.0
                    if p > 0:
                        keep = torch.empty((B * N, D), dtype=torch.uint8, device=dev).bernoulli_(1 - p)
                        scale = 1.0 / (1.0 - p)
                    h, _, dist = LayerTailFn.apply(pre_a, pre_b, keep, scale, score_func.weight, score_func.bias, mask)
                    return dist, h.view(B, N, D)
                # ReasonGNNLayer._forward_autograd, native unfused form, from the two products on
                h = F.relu(pre_a + pre_b).view(B, N, D)
                score = score_func(linear_drop(h)).squeeze(dim=2) + (1 - mask) * VERY_NEG_NUMBER
                return softmax_d1(score), h

            def step(it):
                pre_a.grad = pre_b.grad = None
                score_func.zero_grad(set_to_none=True)
                dist, h = tail()
                loss = (dist * G_d).sum() + (h * G_h).sum()
                loss.backward()
                kept["loss"] = loss.detach()

            ms = _timed(torch, step, a.warm + a.iters, a.warm)
            rec = {"what": "layer_tail_fwd_bwd", "switch": "on" if on else "off", "B": B, "N": N, "D": D, "p": p,
                   "event_ms": _median(ms), "event_ms_min": min(ms), "event_ms_max": max(ms), "iters": a.iters, "warm": a.warm,
                   "loss_last": float(kept["loss"]), "pre_grad_checksum": float(pre_a.grad.double().abs().sum()),
                   "weight_grad_checksum": float(score_func.weight.grad.double().abs().sum()), "device": name}
            print(TAG + json.dumps(rec), flush=True)
            if not on:
                continue
            with torch.no_grad():
                keep = torch.empty((B * N, D), dtype=torch.uint8, device=dev).bernoulli_(1 - p) if p > 0 else None
                scale = 1.0 / (1.0 - p) if p > 0 else 1.0
                w, b = score_func.weight.detach().reshape(-1).contiguous(), score_func.bias.detach()
                A, Bm = pre_a.detach(), pre_b.detach()
                h, score, dist = ops.layer_tail_train(A, Bm, keep, scale, w, b, mask)
                g_h = G_h.view(B * N, D)

                def many(fn):
                    def run(it):
                        for _ in range(REPEAT):
                            fn()
                    return run

                fwd = _median(_timed(torch, many(lambda: ops.layer_tail_train(A, Bm, keep, scale, w, b, mask)),
                                     a.warm + a.iters, a.warm)) / REPEAT
                soft = _median(_timed(torch, many(lambda: ops.masked_softmax(score, B, N)), a.warm + a.iters, a.warm)) / REPEAT
                bwd = _median(_timed(torch, many(lambda: ops.layer_tail_backward(h, dist, keep, scale, w, g_h, G_d)),
                                     a.warm + a.iters, a.warm)) / REPEAT
            elems = B * N * D
            fwd_bytes = elems * (3 * 4 + (1 if p > 0 else 0))
            bwd_bytes = elems * (3 * 4 + (1 if p > 0 else 0))
            row = fwd - soft
            rec = {"what": "row_kernels_by_event_difference", "B": B, "N": N, "D": D, "p": p,
                   "forward_two_launches_ms": fwd, "masked_softmax_ms": soft, "k_lt_fwd_ms": row,
                   "k_lt_fwd_bytes": fwd_bytes, "k_lt_fwd_TBps": (fwd_bytes / (row * 1e-3) / 1e12) if row > 0 else None,
                   "backward_three_launches_ms": bwd, "k_lt_bwd_bytes": bwd_bytes,
                   "k_lt_bwd_TBps_lower_bound": bwd_bytes / (bwd * 1e-3) / 1e12, "copy_ceiling_TBps": COPY_CEILING_TBS,
                   "fits_last_level_cache": 3 * elems * 4 < 256 * 1024 * 1024, "calls_per_event_pair": REPEAT,
                   "iters": a.iters, "warm": a.warm, "device": name}
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "layer_tail_train_time.jsonl"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--only-batch", type=int, default=0, help="with --child: this batch size only (for a profiler run)")
    a = ap.parse_args()
    if a.child:
        return child(a)
    common = ["--child", "--iters", str(a.iters), "--warm", str(a.warm)]
    lines = []
    # a failing child ends the run: nothing more is started on the device after it
    for switch in ("0", "1"):
        _spawn(common, {"GNNRAG_HIP_LAYER_TAIL_TRAIN": switch}, lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
