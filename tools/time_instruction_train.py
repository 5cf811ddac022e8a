#!/usr/bin/env python
"""Instruction generation under autograd with ``GNNRAG_HIP_INSTRUCTION_TRAIN`` off (the reference's torch ops and autograd's
backward of them) and on (``autograd.InstructionsFn``: ``gnnrag_instructions_train`` / ``gnnrag_instructions_backward``), each
setting in a process of its own under its own time limit; ``GNNRAG_HIP_INSTRUCTION=1`` in both:

    python tools/time_instruction_train.py [--iters 20] [--warm 5] [--dropout 0.2] [--out profiles/instruction_train_time.jsonl]

* the module sequence: a stand-in encoder (tests/instruction_oracle.py: an LSTM and the step's linears, random parameters,
  ``linear_drop`` at the reference's default 0.2, training mode, ``install.swap_lstm`` applied in BOTH settings) runs the
  ReaRev call sequence - ``instr(q)``, ``instr.init_reason(q)``, ``get_instruction(instr.relational_ins, i)`` for every
  step (rearev.py:138,192-196) - and one backward of a loss over every result; shapes (B, T, D, I) = (16, 12, 200, 2) and
  (64, 12, 200, 2);
* where oracle/_ref is staged: one whole training step of the reference's trainer (``Trainer_KBQA.train_epoch``,
  train_model.py:209-233: zero_grad, forward, backward, clip, Adam) set up as tools/time_train_step.py does, plus
  ``install.patch_instruction``; variant d200, batch 16.

HIP events around each iteration (stream time: what the device needed, or the host where the host is slower), median of
``--iters`` after ``--warm``.  One JSON line per measurement, printed and appended to ``--out``.  With dropout active the two
settings draw different random numbers: the times compare, the losses do not."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(16, 12, 200, 2), (64, 12, 200, 2)]
TAG = "GNNRAG_INSTR_TRAIN "
CHILD_LIMIT_S = 300


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


def child_module(a):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import numpy as np
    import torch
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import autograd, install
    from gnnrag_amd.modules.question_encoding.instruction import patch_instruction, train_enabled
    import instruction_oracle as io
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_instruction_train.py needs a GPU")
    dev = torch.device("cuda", 0)
    calls = {"n": 0}
    apply = autograd.InstructionsFn.apply

    def counted(*args):
        calls["n"] += 1
        return apply(*args)

    autograd.InstructionsFn.apply = counted
    for B, T, D, I in SHAPES:
        torch.manual_seed(B + D)
        mod = io.make_standin(300, D, I, num_word=1000, linear_dropout=a.dropout, device=dev).train()
        install.swap_lstm(mod)
        patch_instruction(mod)
        rng = np.random.default_rng(B)
        text = rng.integers(0, 1000, (B, T))
        text[np.arange(T)[None, :] >= rng.integers(3, T + 1, B)[:, None]] = 1000
        q = torch.from_numpy(text).long().to(dev)
        losses = []

        def sequence(it):
            mod.zero_grad(set_to_none=True)
            ins, _ = mod(q)
            loss = sum(t.sum() for t in ins)
            mod.init_reason(q)
            for i in range(mod.num_ins):
                r, _ = mod.get_instruction(mod.relational_ins, step=i)
                mod.instructions.append(r.unsqueeze(1))
                mod.relational_ins = r
                loss = loss + (r * r).sum()
            loss.backward()
            losses.append(loss.detach())

        calls["n"] = 0
        ms = _timed(torch, sequence, a.warm + a.iters, a.warm)
        rec = {"what": "module_sequence_fwd_bwd", "switch": "on" if train_enabled() else "off", "B": B, "T": T, "D": D, "I": I,
               "linear_dropout": a.dropout, "event_ms": _median(ms), "event_ms_min": min(ms), "event_ms_max": max(ms),
               "iters": a.iters, "warm": a.warm, "instructions_fn_calls_per_sequence": calls["n"] / (a.warm + a.iters),
               "loss_last": float(losses[-1]), "grad_checksum": float(mod.cq_linear.weight.grad.double().abs().sum()),
               "device": torch.cuda.get_device_name(0)}
        print(TAG + json.dumps(rec), flush=True)


def child_step(a):
    """The reference's trainer on the staged data, set up as tools/time_train_step.py does."""
    ref = os.path.join(REPO, "oracle", "_ref", "gnn")
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
    from gnnrag_amd.modules.question_encoding.instruction import train_enabled
    install.install()
    install.limit_host_threads()
    import parsing
    from train_model import Trainer_KBQA
    from utils import create_logger
    variant, batch = "d200", 16
    parser = argparse.ArgumentParser()
    parsing.add_parse_args(parser)
    argv = list(stage_ref.variant_argv(variant))
    argv[argv.index("--batch_size") + 1] = str(batch)
    ck = tempfile.mkdtemp(prefix="gnnrag_instr_train_") + "/"
    args = parser.parse_args(argv + ["--checkpoint_dir", ck, "--experiment_name", "timing"])
    args.use_cuda = True
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    tr = Trainer_KBQA(args=vars(args), model_name=args.model_name, logger=create_logger(args))
    tr.load_ckpt(os.path.join(stage_ref.CKPT, stage_ref.ckpt_name(variant)))
    from gnnrag_amd.data.fact_mat import patch_loader
    patch_loader(tr.train_data, cache=False, keep_rng_stream=True)
    install.swap_lstm(tr.model)
    install.patch_instruction(tr.model)
    tr.model.train()
    tr.train_data.reset_batches(is_sequential=False)
    n = a.warm + a.iters
    batches = [tr.train_data.get_batch(it, tr.args["batch_size"], tr.args["fact_drop"]) for it in range(n)]
    losses = []

    def step(it):
        tr.optim_model.zero_grad()
        loss, _, _, _ = tr.model(batches[it], training=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_([p for _, p in tr.model.named_parameters()], tr.args["gradient_clip"])
        tr.optim_model.step()
        losses.append(loss.detach())

    ms = _timed(torch, step, n, a.warm)
    rec = {"what": "train_step", "switch": "on" if train_enabled() else "off", "variant": variant, "batch": batch,
           "entity_dim": int(tr.args["entity_dim"]), "num_ins": int(tr.args["num_ins"]),
           "linear_dropout": float(tr.args["linear_dropout"]), "event_ms": _median(ms), "event_ms_min": min(ms),
           "event_ms_max": max(ms), "iters": a.iters, "warm": a.warm, "losses": [float(x) for x in losses],
           "hip_lstm_train": os.environ.get("GNNRAG_HIP_LSTM_TRAIN", "default"), "device": torch.cuda.get_device_name(0)}
    print(TAG + json.dumps(rec), flush=True)
    import shutil
    shutil.rmtree(ck, ignore_errors=True)


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
    ap.add_argument("--dropout", type=float, default=0.2)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "instruction_train_time.jsonl"))
    ap.add_argument("--child", choices=["module", "step"])
    a = ap.parse_args()
    if a.child:
        return {"module": child_module, "step": child_step}[a.child](a)
    common = ["--iters", str(a.iters), "--warm", str(a.warm), "--dropout", str(a.dropout)]
    staged = os.path.isfile(os.path.join(REPO, "oracle", "_ref", "gnn", "main.py"))
    lines = []
    # a failing child ends the run: nothing more is started on the device after it
    for switch in ("0", "1"):
        env = {"GNNRAG_HIP_INSTRUCTION": "1", "GNNRAG_HIP_INSTRUCTION_TRAIN": switch}
        _spawn(["--child", "module"] + common, env, lines)
        if staged and not a.no_step:
            _spawn(["--child", "step"] + common, env, lines)
    if not staged:
        lines.append({"what": "train_step", "skipped": "oracle/_ref not staged"})
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
