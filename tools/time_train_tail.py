#!/usr/bin/env python
"""Times what follows the last ``dist`` of a training forward (rearev.py:227-243) with ``GNNRAG_HIP_LOSS_METRICS`` off (the
wrapped methods: the torch ops of ``get_loss_kl`` with autograd's backward, ``calc_h1`` and the host loop of ``calc_f1_new``)
and on (``autograd.KLLossFn`` and one ``gnnrag_train_metrics`` call), in separate processes of one session:

    python tools/time_train_tail.py [--iters 20] [--warm 5] [--out profiles/train_tail_time.jsonl]

The timed sequence is ``calc_loss_label`` -> ``backward`` -> ``get_eval_metric`` -> the two ``.tolist()`` of the forward, on a
stand-in model patched by ``modules.train_tail.patch_loss_metrics``, at (B, N) = (16, 2000) and (64, 2000) with the share of
questions whose H@1 is 1 set to 0, 0.5 and 1 (``tests/train_tail_oracle.timing_case``).  Reported per leg: host wall time up
to the last ``.tolist()`` (``perf_counter``) and stream time (HIP events), each the median of ``--iters`` after ``--warm``.

The stand-in's own methods make the reference's calls in the reference's order - the torch ops of base_model.py:193-215 and
:287-292, then per question with a hit one ``.item()`` and four ``.tolist()`` of N-vectors, the Python loop over the N slots
and the sort (base_model.py:249-285) - so that the switch-off leg pays what the reference pays.
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(16, 2000), (64, 2000)]
HIT_SHARES = [0.0, 0.5, 1.0]
TAG = "GNNRAG_TRAIN_TAIL "
CHILD_LIMIT_S = 300


def _median(xs):
    xs = sorted(xs)
    n = len(xs)
    return xs[n // 2] if n % 2 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])


def make_model(torch, oracle, c, dev):
    F = torch.nn.functional

    class Model:
        loss_type, eps, num_entity, device = "kl", c["eps"], c["pad_id"], dev
        seed_entities = torch.from_numpy(c["seed"]).to(dev).requires_grad_(True)
        local_entity = torch.from_numpy(c["local_entity"]).to(dev)

        def calc_loss_label(self, curr_dist, teacher_dist, label_valid):
            answer_len = torch.sum(teacher_dist, dim=1, keepdim=True)
            answer_len[answer_len == 0] = 1.0
            tp_loss = F.kl_div(torch.log(curr_dist + 1e-8), teacher_dist.div(answer_len), reduction="none")
            return torch.sum(tp_loss * label_valid) / curr_dist.size(0)

        def get_eval_metric(self, pred_dist, answer_dist):
            with torch.no_grad():
                greedy = pred_dist.argmax(dim=-1, keepdim=True)
                top1 = torch.zeros_like(pred_dist).scatter_(1, greedy, 1.0)
                h1 = (torch.sum(top1 * (answer_dist > 1e-10).float(), dim=-1) > 0).float()
                f1_list = []
                for b in range(pred_dist.size(0)):
                    if h1[b].item() == 0.0:
                        f1_list.append(0.0)
                        continue
                    ents, probs = self.local_entity[b, :].tolist(), pred_dist[b, :].tolist()
                    ans, seeds = answer_dist[b, :].tolist(), self.seed_entities[b, :].tolist()
                    f1_list.append(oracle.question_metrics(probs, ans, seeds, ents, self.num_entity, self.eps)[2])
                return h1, torch.FloatTensor(f1_list).to(self.device)

    return Model()


def child(a):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import torch
    import gnnrag_amd  # noqa: F401
    import train_tail_oracle as oracle
    from gnnrag_amd import ops
    from gnnrag_amd.modules.train_tail import enabled, patch_loss_metrics
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_train_tail.py needs a GPU")
    dev = torch.device("cuda", 0)
    name = torch.cuda.get_device_name(0)
    calls = {"n": 0}
    inner = ops.train_metrics

    def counted(*args, **kw):
        calls["n"] += 1
        return inner(*args, **kw)

    ops.train_metrics = counted
    for B, N in SHAPES:
        for share in HIT_SHARES:
            c = oracle.timing_case(B, N, share, seed=B)
            model = patch_loss_metrics(make_model(torch, oracle, c, dev))
            pred = torch.from_numpy(c["pred"]).to(dev).requires_grad_(True)
            answer, valid = torch.from_numpy(c["answer"]).to(dev), torch.from_numpy(c["label_valid"]).to(dev)
            host_ms, event_ms, last = [], [], None
            calls["n"] = 0
            for it in range(a.warm + a.iters):
                pred.grad = None
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                loss = model.calc_loss_label(curr_dist=pred, teacher_dist=answer, label_valid=valid)
                loss.backward()
                h1, f1 = model.get_eval_metric(pred, answer)
                last = [h1.tolist(), f1.tolist()]
                t1 = time.perf_counter()
                e1.record()
                e1.synchronize()
                if it >= a.warm:
                    host_ms.append((t1 - t0) * 1e3)
                    event_ms.append(e0.elapsed_time(e1))
            rec = {"what": "loss_backward_metrics_tolist", "switch": "on" if enabled() else "off", "B": B, "N": N,
                   "hit_share": share, "host_ms": _median(host_ms), "host_ms_min": min(host_ms), "host_ms_max": max(host_ms),
                   "event_ms": _median(event_ms), "event_ms_min": min(event_ms), "iters": a.iters, "warm": a.warm,
                   "train_metrics_calls_per_step": calls["n"] / float(a.warm + a.iters), "loss_last": float(loss.detach()),
                   "h1_sum": sum(last[0]), "f1_sum": sum(last[1]),
                   "grad_checksum": float(pred.grad.double().abs().sum()), "device": name}
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "train_tail_time.jsonl"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    common = ["--child", "--iters", str(a.iters), "--warm", str(a.warm)]
    lines = []
    # a failing child ends the run: nothing more is started on the device after it
    for switch in ("0", "1"):
        _spawn(common, {"GNNRAG_HIP_LOSS_METRICS": switch}, lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
