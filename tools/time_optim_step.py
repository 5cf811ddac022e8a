#!/usr/bin/env python
"""Times the two statements that end a training step (train_model.py:228-230) - ``clip_grad_norm_`` over the parameters and
``Adam.step()`` - with ``GNNRAG_HIP_OPTIM`` off (torch's own: the reference's statements on an optimiser patched by
``gnnrag_amd.optim.patch_adam``) and on (``optimizer.clip_and_step``: three launches), in separate processes of one session,
two rounds of (off, on) so that the spread between two runs of one leg can be read next to the difference between the legs:

    python tools/time_optim_step.py [--iters 20] [--warm 5] [--rounds 2] [--out profiles/optim_step_time.jsonl]

Parameter lists:
  d200      every tensor of the staged d200 checkpoint (tests/golden/ckpt/synth200-final.ckpt): the model's own 55 tensors;
  released  the same layer tensors with the vocabulary tables at the released sizes: the two word tables [7000, 300] and the
            two relation tables [6106, 200] in place of the synthetic dataset's small ones.
Gradients are random with a total norm of 3 (``gradient_clip`` is 1: the clip acts).  Reported per leg and list: host wall
time of the statements (``perf_counter``: what the host-bound step pays) and stream time (HIP events), each the median of
``--iters`` after ``--warm``, and the number of steps the library took (0 in the off leg, every step in the on leg).
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CKPT = os.path.join(REPO, "tests", "golden", "ckpt", "synth200-final.ckpt")
RELEASED = {"word_embedding.weight": (7000, 300), "instruction.word_embedding.weight": (7000, 300),
            "relation_embedding.weight": (6106, 200), "relation_embedding_inv.weight": (6106, 200)}
TAG = "GNNRAG_OPTIM_STEP "
CHILD_LIMIT_S = 300
MAX_NORM = 1.0


def _median(xs):
    xs = sorted(xs)
    n = len(xs)
    return xs[n // 2] if n % 2 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])


def shape_lists(torch):
    sd = torch.load(CKPT, map_location="cpu", weights_only=False)["model_state_dict"]
    d200 = [(k, tuple(v.shape)) for k, v in sd.items() if v.dtype == torch.float32]
    return {"d200": d200, "released": [(k, RELEASED.get(k, s)) for k, s in d200]}


def child(a):
    sys.path.insert(0, REPO)
    import torch
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd.optim import enabled, patch_adam
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_optim_step.py needs a GPU")
    dev = torch.device("cuda", 0)
    name = torch.cuda.get_device_name(0)
    on = enabled()
    for which, shapes in shape_lists(torch).items():
        gen = torch.Generator().manual_seed(0)
        params = [torch.nn.Parameter((torch.randn(*s, generator=gen) * 0.1).to(dev)) for _, s in shapes]
        grads = [torch.randn(*s, generator=gen) for _, s in shapes]
        total = sum(float((g.double() ** 2).sum()) for g in grads) ** 0.5
        grads = [(g * (3.0 / total)).to(dev) for g in grads]
        opt = patch_adam(torch.optim.Adam(params, lr=5e-4))
        host_ms, event_ms, norm = [], [], None
        for it in range(a.warm + a.iters):
            for p, g in zip(params, grads):
                p.grad = g.clone()                       # clip_grad_norm_ rescales .grad in place: a fresh copy every step
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            if on:
                norm = opt.clip_and_step(params, MAX_NORM)
            else:
                norm = torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
                opt.step()
            t1 = time.perf_counter()
            e1.record()
            e1.synchronize()
            if it >= a.warm:
                host_ms.append((t1 - t0) * 1e3)
                event_ms.append(e0.elapsed_time(e1))
        rec = {"what": "clip_grad_norm_and_adam_step", "switch": "on" if on else "off", "params": which,
               "tensors": len(params), "elements": sum(p.numel() for p in params), "round": a.round,
               "host_ms": _median(host_ms), "host_ms_min": min(host_ms), "host_ms_max": max(host_ms),
               "event_ms": _median(event_ms), "event_ms_min": min(event_ms), "iters": a.iters, "warm": a.warm,
               "library_steps": opt._gnnrag_optim.calls, "total_norm_last": float(norm),
               "param_checksum": float(sum(p.detach().double().abs().sum() for p in params)), "device": name}
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
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--round", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "optim_step_time.jsonl"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    lines = []
    # a failing child ends the run: nothing more is started on the device after it
    for rnd in range(a.rounds):
        for switch in ("0", "1"):
            _spawn(["--child", "--iters", str(a.iters), "--warm", str(a.warm), "--round", str(rnd + 1)],
                   {"GNNRAG_HIP_OPTIM": switch}, lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
