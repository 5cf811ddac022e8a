#!/usr/bin/env python
"""Relation-text features (``get_rel_feature`` with ``--relation_word_emb True``) with ``GNNRAG_HIP_REL_TEXT`` off (the
reference's torch ops: the path of the tree before ``gnnrag_rel_text_pool`` existed) and on (``patch_rel_feature``: one
fused call, forward and backward), each setting in a process of its own:

    python tools/time_rel_text.py [--iters 20] [--warm 5] [--rounds 2] [--R 6106] [--T 20] [--out profiles/rel_text_time.jsonl]
    python tools/time_rel_text.py --kernel [--libs 256=,128=gnn-rag_amd/lib/exp_rt128.so,...]

A stand-in model (tests/rel_text_oracle.py: ``question_emb``, the repo's ``AttnEncoder``, random LM states for R relation
texts of T tokens, both directions as in ReaRev) runs ``get_rel_feature`` under ``no_grad`` (forward only) and under
autograd followed by ``backward()`` of a weighted sum of both outputs (forward + backward), at (K, D) = (384, 50) and
(768, 200).  T = 20 is inferred from the 18.8 GFLOP that ``install.cache_rel_features`` quotes for WebQSP's relations, not
read from data: hence an option.  Per iteration ``perf_counter`` around the calls = host enqueue time, HIP events around them
= stream time; median of ``--iters`` after ``--warm``; ``--rounds`` repeats the off / on pair (spread).  The checksums of
the outputs and gradients let the two settings be compared.  One JSON line per measurement, printed and appended to ``--out``.

``--kernel``: ``ops.rel_text_pool`` (saving) and ``ops.rel_text_pool_backward`` alone, per library given in ``--libs`` as
``label=path`` (``GNNRAG_LIB``; empty path = the built library): the workgroup-size sweep of the streaming kernels
(``-DGNNRAG_RT_THREADS``, ``build.build_variant``), with the bytes of X over the time as a rate."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KD = [(384, 50), (768, 200)]
TAG = "GNNRAG_RELTEXT "


def _median(xs):
    xs = sorted(xs)
    n = len(xs)
    return xs[n // 2] if n % 2 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])


def _measure(torch, fn, iters, warm):
    host, dev = [], []
    for it in range(warm + iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        e1.record()
        e1.synchronize()
        if it >= warm:
            host.append((t1 - t0) * 1e3)
            dev.append(e0.elapsed_time(e1))
    return {"host_ms": _median(host), "event_ms": _median(dev), "host_ms_min": min(host), "event_ms_min": min(dev)}


def _setup():
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import torch
    import gnnrag_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_rel_text.py needs a GPU")
    return torch, torch.device("cuda", 0)


def child_module(a):
    torch, dev = _setup()
    from gnnrag_amd import ops
    from gnnrag_amd.modules.rel_text import enabled, patch_rel_feature
    import rel_text_oracle as ro
    count = {"rel_text_pool": 0, "rel_text_pool_backward": 0}
    for name in count:
        def counted(*args, _f=getattr(ops, name), _n=name, **kw):
            count[_n] += 1
            return _f(*args, **kw)
        setattr(ops, name, counted)
    for K, D in KD:
        torch.manual_seed(K + D)
        mod = patch_rel_feature(ro.make_standin(a.R, a.T, K, D, directions=2, seed=K, device=dev), 2)
        gs = [torch.randn(a.R, D, device=dev) for _ in range(2)]
        params = [mod.instruction.question_emb.weight, mod.instruction.question_emb.bias, mod.self_att_r.attn_linear.weight]
        last = {}

        def forward():
            with torch.no_grad():
                last["out"] = mod.get_rel_feature()

        def train():
            for p in params:
                p.grad = None
            out = mod.get_rel_feature()
            ((out[0] * gs[0]).sum() + (out[1] * gs[1]).sum()).backward()
            last["out"] = out

        for what, fn in (("forward", forward), ("forward_backward", train)):
            for k in count:
                count[k] = 0
            rec = _measure(torch, fn, a.iters, a.warm)
            rec.update({"what": what, "switch": "on" if enabled() else "off", "R": a.R, "T": a.T, "K": K, "D": D,
                        "directions": 2, "iters": a.iters, "warm": a.warm,
                        "library_calls_per_iteration": {k: v / (a.iters + a.warm) for k, v in count.items()},
                        "out_checksum": [float(o.double().sum()) for o in last["out"]],
                        "grad_checksum": [float(p.grad.double().sum()) for p in params] if what != "forward" else None,
                        "device": torch.cuda.get_device_name(0)})
            print(TAG + json.dumps(rec), flush=True)
        del mod, gs, params, last
        torch.cuda.empty_cache()


def child_kernel(a):
    torch, dev = _setup()
    from gnnrag_amd import ops
    import rel_text_oracle as ro
    for K, D in KD:
        c = ro.random_case(a.R, a.T, K, D, seed=K)
        t = lambda x: torch.from_numpy(x).to(dev)      # noqa: E731
        Xf, Xi, mask, W, b, w_a, gf, gi = (t(x) for x in c["Xs"] + [c["mask"], c["W"], c["b"], c["a"]] + c["gs"])
        keep = {}

        def fwd():
            keep["r"] = ops.rel_text_pool(Xf, Xi, mask, W, b, w_a, save=True)

        def bwd():
            keep["g"] = ops.rel_text_pool_backward(Xf, Xi, W, w_a, keep["r"][2], keep["r"][3], gf, gi)

        x_bytes = 2 * Xf.numel() * 4
        for what, fn in (("pool", fwd), ("pool_backward", bwd)):
            rec = _measure(torch, fn, a.iters, a.warm)
            rec.update({"what": "kernel_" + what, "threads": a.label, "R": a.R, "T": a.T, "K": K, "D": D, "directions": 2,
                        "iters": a.iters, "x_bytes": x_bytes, "x_gb_per_s_event": x_bytes / rec["event_ms"] * 1e-6,
                        "checksum": float(sum(o.double().sum() for o in (keep["r"][:2] if what == "pool" else keep["g"]))),
                        "device": torch.cuda.get_device_name(0)})
            print(TAG + json.dumps(rec), flush=True)


def _spawn(argv, env_extra, lines):
    env = dict(os.environ)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, env=env, capture_output=True, text=True)
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
    ap.add_argument("--R", type=int, default=6106)
    ap.add_argument("--T", type=int, default=20)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--libs", default="256=")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rel_text_time.jsonl"))
    ap.add_argument("--child", choices=["module", "kernel"])
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.child:
        return {"module": child_module, "kernel": child_kernel}[a.child](a)
    common = ["--iters", str(a.iters), "--warm", str(a.warm), "--R", str(a.R), "--T", str(a.T)]
    lines = []
    if a.kernel:
        for spec in a.libs.split(","):
            label, _, path = spec.partition("=")
            env = {"GNNRAG_LIB": os.path.abspath(os.path.join(REPO, path))} if path else {}
            _spawn(["--child", "kernel", "--label", label] + common, env, lines)
    else:
        for rnd in range(a.rounds):
            for switch in ("0", "1"):
                before = len(lines)
                _spawn(["--child", "module"] + common, {"GNNRAG_HIP_REL_TEXT": switch}, lines)
                for rec in lines[before:]:
                    rec["round"] = rnd
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
