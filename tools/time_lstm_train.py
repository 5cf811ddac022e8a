#!/usr/bin/env python
"""Forward + backward of the question encoder's LSTM ALONE, in training: ``HipLSTM`` on the library
(``GNNRAG_HIP_LSTM_TRAIN=1``: gnnrag_lstm_forward_train / gnnrag_lstm_backward) against its parent class
(``torch.nn.LSTM`` = MIOpen's RNN calls), in one process, on HIP events:

    python tools/time_lstm_train.py [--T 9 --E 300] [--iters 20] [--warm 5] [--out profiles/lstm_train_time.jsonl]

One measured iteration is what the encoder does per training call: zero [1,B,H] states without grad, forward, a loss
that uses ``out`` and ``h_n``, ``backward()`` (parameter gradients and dx).  Shapes: hidden size 200 and 50, batch 16
and 64; T (longest question of the train split) and E (width of word_emb.npy) are read from the staged dataset
(oracle/_ref/data/synth12) when it is there, else T = 9, E = 300; ``--T`` / ``--E`` override.  Median of ``--iters``
after ``--warm``; the two forms alternate inside every iteration so that clock drift hits both alike.  One JSON line per
shape is printed and appended to ``--out``."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def staged_shape():
    folder = os.path.join(REPO, "oracle", "_ref", "data", "synth12")
    try:
        import numpy as np
        E = int(np.load(os.path.join(folder, "word_emb.npy"), mmap_mode="r").shape[1])
        T = 0
        with open(os.path.join(folder, "train.json")) as f:
            for line in f:
                T = max(T, len(json.loads(line)["question"].split()))
        if T > 0 and E > 0:
            return T, E, "staged dataset (oracle/_ref/data/synth12)"
    except (OSError, KeyError, ValueError):
        pass
    return 9, 300, "default"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=0)
    ap.add_argument("--E", type=int, default=0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lstm_train_time.jsonl"))
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    import numpy as np
    import torch
    import torch.nn as nn
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd.modules.question_encoding.lstm import HipLSTM
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_lstm_train.py needs a GPU")
    dev = torch.device("cuda", 0)
    T, E, source = staged_shape()
    if a.T > 0 or a.E > 0:
        T, E, source = a.T or T, a.E or E, "command line"

    def step(mod, x, zeros, w_out, w_h):
        mod.zero_grad(set_to_none=True)
        x.grad = None
        out, (h_n, _) = mod(x, (zeros, zeros))
        ((out * w_out).sum() + (h_n * w_h).sum()).backward()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    lines = []
    for H in (200, 50):
        for B in (16, 64):
            torch.manual_seed(B + H)
            parent = nn.LSTM(E, H, batch_first=True).to(dev).train()
            hip = HipLSTM.sharing(parent)
            x = torch.randn(B, T, E, device=dev, requires_grad=True)
            zeros = torch.zeros(1, B, H, device=dev)
            w_out, w_h = torch.randn(B, T, H, device=dev), torch.randn(1, B, H, device=dev)
            ms = {"hip": [], "parent": []}
            for it in range(a.warm + a.iters):
                for name, mod, switch in (("hip", hip, "1"), ("parent", hip, "0")):
                    os.environ["GNNRAG_HIP_LSTM_TRAIN"] = switch       # "0": HipLSTM.forward hands over to nn.LSTM.forward
                    t = timed(lambda: step(mod, x, zeros, w_out, w_h))
                    if it >= a.warm:
                        ms[name].append(t)
            # both forms derive the same gradients (a sanity check of what was timed, not a test)
            os.environ["GNNRAG_HIP_LSTM_TRAIN"] = "1"
            step(hip, x, zeros, w_out, w_h)
            g_hip = parent.weight_ih_l0.grad.clone()
            os.environ["GNNRAG_HIP_LSTM_TRAIN"] = "0"
            step(hip, x, zeros, w_out, w_h)
            g_par = parent.weight_ih_l0.grad
            rel = float((g_hip - g_par).abs().max() / g_par.abs().max())
            rec = {"B": B, "T": T, "E": E, "H": H, "shape_from": source, "iters": a.iters, "warm": a.warm,
                   "hip_ms": float(np.median(ms["hip"])), "hip_ms_min": float(min(ms["hip"])),
                   "parent_ms": float(np.median(ms["parent"])), "parent_ms_min": float(min(ms["parent"])),
                   "dw_ih_rel_diff_hip_vs_parent": rel, "device": torch.cuda.get_device_name(0)}
            rec["speedup"] = rec["parent_ms"] / rec["hip_ms"]
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
