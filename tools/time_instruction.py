#!/usr/bin/env python
"""Instruction generation with ``GNNRAG_HIP_INSTRUCTION`` off (the reference's torch ops: the path of the tree before
``gnnrag_instructions`` existed) and on (``patch_instruction``: one launch for all steps, the second pass of a forward
from the first), each setting in a process of its own:

    python tools/time_instruction.py [--iters 20] [--warm 5] [--rounds 2] [--out profiles/instruction_time.jsonl]
    python tools/time_instruction.py --kernel [--libs 512=,256=lib/exp_ins256.so,...]

* the module alone: a stand-in encoder (tests/instruction_oracle.py: an LSTM and the step's three linears, random
  parameters, ``install.swap_lstm`` applied in BOTH settings) runs the ReaRev call sequence - ``instr(q)``,
  ``instr.init_reason(q)``, ``get_instruction(instr.relational_ins, i)`` for every step (rearev.py:138,192-196) - on a NEW
  question tensor every iteration, as an evaluation loop does; shapes (B, T, D, I) = (1, 12, 50, 3), (16, 12, 200, 2),
  (64, 12, 200, 2);
* a whole forward of the reference's own model as tools/run_reference.py sets it up (``install.install()``,
  ``swap_lstm``, ``patch_instruction``) on the staged dataset and checkpoint, where oracle/_ref is staged: variant d50
  at batch 1, d200 at batch 64.

Per iteration: ``perf_counter`` around the calls = host enqueue time (the device is idle before, nothing waits inside), HIP
events around them = stream time (what the device needed, or the host where the host is slower).  Median of ``--iters``
after ``--warm``.  ``--rounds`` repeats the off / on pair (spread).  One JSON line per measurement, printed and written
to ``--out``.

``--kernel``: ``gnnrag_instructions`` alone, 20 calls captured into one graph and replayed (device time per call without
host gaps), per library given in ``--libs`` as ``label=path`` (``GNNRAG_LIB``; empty path = the built library): how the
workgroup size (``-DGNNRAG_INS_THREADS``, ``build.build_variant``) was chosen."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 12, 50, 3), (16, 12, 200, 2), (64, 12, 200, 2)]
FORWARDS = [("d50", 1), ("d200", 64)]
TAG = "GNNRAG_INSTR "


def _median(xs):
    xs = sorted(xs)
    n = len(xs)
    return xs[n // 2] if n % 2 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])


def _measure(torch, fn, inputs, warm):
    """fn(x) for every x of inputs; (host ms, event ms) medians over inputs[warm:]."""
    host, dev = [], []
    for it, x in enumerate(inputs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        fn(x)
        t1 = time.perf_counter()
        e1.record()
        e1.synchronize()
        if it >= warm:
            host.append((t1 - t0) * 1e3)
            dev.append(e0.elapsed_time(e1))
    return _median(host), _median(dev), min(host), min(dev)


def child_module(a):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import numpy as np
    import torch
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import install, ops
    from gnnrag_amd.modules.question_encoding.instruction import enabled, patch_instruction
    import instruction_oracle as io
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_instruction.py needs a GPU")
    dev = torch.device("cuda", 0)
    count = {"instructions": 0, "lstm_forward": 0}
    for name in count:
        def counted(*args, _f=getattr(ops, name), _n=name, **kw):
            count[_n] += 1
            return _f(*args, **kw)
        setattr(ops, name, counted)
    for B, T, D, I in SHAPES:
        torch.manual_seed(B + D)
        mod = io.make_standin(300, D, I, num_word=1000, device=dev).eval()
        install.swap_lstm(mod)
        patch_instruction(mod)
        rng = np.random.default_rng(B)
        text = rng.integers(0, 1000, (B, T))
        text[np.arange(T)[None, :] >= rng.integers(3, T + 1, B)[:, None]] = 1000
        q0 = torch.from_numpy(text).long().to(dev)
        qs = [q0.clone() for _ in range(a.warm + a.iters)]

        def sequence(q):
            with torch.no_grad():
                mod(q)
                mod.init_reason(q)
                for i in range(mod.num_ins):
                    r, _ = mod.get_instruction(mod.relational_ins, step=i)
                    mod.instructions.append(r.unsqueeze(1))
                    mod.relational_ins = r

        count["instructions"] = count["lstm_forward"] = 0
        host, ev, host_min, ev_min = _measure(torch, sequence, qs, a.warm)
        launches = {k: v / len(qs) for k, v in count.items()}
        last = torch.stack([t.squeeze(1) for t in mod.instructions]).double().cpu().numpy()
        with torch.no_grad():
            mod(qs[-1].clone())
        want, _ = io.standin_oracle(mod)
        rec = {"what": "module_sequence", "switch": "on" if enabled() else "off", "B": B, "T": T, "D": D, "I": I,
               "host_ms": host, "event_ms": ev, "host_ms_min": host_min, "event_ms_min": ev_min, "iters": a.iters,
               "warm": a.warm, "lstm_launches_per_sequence": launches["lstm_forward"],
               "instruction_launches_per_sequence": launches["instructions"],
               "max_abs_diff_vs_float64_oracle": float(np.abs(last - want).max()),
               "device": torch.cuda.get_device_name(0)}
        print(TAG + json.dumps(rec), flush=True)


def child_forward(a):
    """The reference's model on the staged data, set up as tools/run_reference.py does (cf. tools/time_train_step.py)."""
    ref = os.path.join(REPO, "oracle", "_ref", "gnn")
    if not os.path.isfile(os.path.join(ref, "main.py")):
        print(TAG + json.dumps({"what": "forward", "skipped": "oracle/_ref not staged"}), flush=True)
        return
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    sys.path.insert(0, ref)
    os.chdir(ref)
    import tempfile
    import numpy as np
    import torch
    import stage_ref
    stage_ref.shim_reference_startup_bugs()
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import install
    from gnnrag_amd.modules.question_encoding.instruction import enabled
    install.install()
    install.limit_host_threads()
    import parsing
    from train_model import Trainer_KBQA
    from utils import create_logger
    for variant, batch in FORWARDS:
        parser = argparse.ArgumentParser()
        parsing.add_parse_args(parser)
        argv = list(stage_ref.variant_argv(variant))
        argv[argv.index("--test_batch_size") + 1] = str(batch)
        ck = tempfile.mkdtemp(prefix="gnnrag_instr_") + "/"
        args = parser.parse_args(argv + ["--checkpoint_dir", ck, "--experiment_name", "timing"])
        args.use_cuda = True
        np.random.seed(args.seed)
        torch.manual_seed(args.seed)
        tr = Trainer_KBQA(args=vars(args), model_name=args.model_name, logger=create_logger(args))
        tr.load_ckpt(os.path.join(stage_ref.CKPT, stage_ref.ckpt_name(variant)))
        install.swap_lstm(tr.model)
        install.patch_instruction(tr.model)
        tr.model.eval()
        data = tr.test_data
        data.reset_batches(is_sequential=True)
        n_batches = max(1, data.num_data // batch)
        batches = [data.get_batch(it % n_batches, batch, fact_dropout=0.0, test=True)[:-1] for it in range(a.warm + a.iters)]
        preds = []

        def forward(b):
            with torch.no_grad():
                preds.append(tr.model(b)[2])

        host, ev, host_min, ev_min = _measure(torch, forward, batches, a.warm)
        rec = {"what": "forward", "switch": "on" if enabled() else "off", "variant": variant, "batch": batch,
               "entity_dim": int(tr.args["entity_dim"]), "num_ins": int(tr.args["num_ins"]), "host_ms": host, "event_ms": ev,
               "host_ms_min": host_min, "event_ms_min": ev_min, "iters": a.iters, "warm": a.warm,
               "pred_dist_checksum": float(sum(float(p.double().square().sum()) for p in preds[a.warm:])),
               "device": torch.cuda.get_device_name(0)}
        print(TAG + json.dumps(rec), flush=True)
        import shutil
        shutil.rmtree(ck, ignore_errors=True)


def child_kernel(a):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import torch
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import ops
    import instruction_oracle as io
    dev = torch.device("cuda", 0)
    calls = 20
    for B, T, D, I in SHAPES:
        c = io.random_case(B, T, D, I, seed=1)
        t = [[torch.from_numpy(x).to(dev) for x in c[k]] if isinstance(c[k], list) else torch.from_numpy(c[k]).to(dev)
             for k in io.ARGS]
        ops.instructions(*t)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(calls):
                out = ops.instructions(*t)
        ms = []
        for it in range(a.warm + a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            if it >= a.warm:
                ms.append(e0.elapsed_time(e1) / calls)
        rec = {"what": "kernel", "threads": a.label, "B": B, "T": T, "D": D, "I": I, "us_per_call": _median(ms) * 1e3,
               "us_per_call_min": min(ms) * 1e3, "calls_per_graph": calls, "iters": a.iters,
               "checksum": float(out[0].double().sum()), "device": torch.cuda.get_device_name(0)}
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
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--libs", default="512=")
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "instruction_time.jsonl"))
    ap.add_argument("--child", choices=["module", "forward", "kernel"])
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.child:
        return {"module": child_module, "forward": child_forward, "kernel": child_kernel}[a.child](a)
    common = ["--iters", str(a.iters), "--warm", str(a.warm)]
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
                _spawn(["--child", "module"] + common, {"GNNRAG_HIP_INSTRUCTION": switch}, lines)
                if not a.no_forward and rnd == 0:
                    _spawn(["--child", "forward"] + common, {"GNNRAG_HIP_INSTRUCTION": switch}, lines)
                for rec in lines[before:]:
                    rec["round"] = rnd
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
