#!/usr/bin/env python
"""The frozen BERT-class question encoder with ``GNNRAG_HIP_LM`` off (transformers' own forward) and on
(``patch_lm_encoder``: ``gnnrag_bert_encode``, 8 launches per layer), each setting in a process of its own, started fresh:

    python tools/time_bert_encoder.py [--arch bert|roberta|mpnet] [--iters 20] [--warm 5] [--rounds 2]
                                      [--out profiles/bert_encoder_time.jsonl]
    python tools/time_bert_encoder.py --kernel [--libs 256=,64=gnn-rag_amd/lib/exp_bertatt64.so,...]
    python tools/time_bert_encoder.py --train [--arch bert|roberta|mpnet]
    python tools/time_bert_encoder.py --splitk [--arch bert|roberta] [--kernel]
                                      [--out profiles/bert_encoder_splitk_time.jsonl]
    python tools/time_bert_encoder.py --finetune [--arch bert|roberta]
                                      [--out profiles/bert_encoder_finetune_time.jsonl]
    python tools/time_bert_encoder.py --finetune --full [--arch bert|roberta|mpnet]
                                      [--out profiles/bert_encoder_finetune_full_time.jsonl]

* the encode: a MiniLM-shaped ``BertModel`` (hidden 384, 12 heads, intermediate 1536, 6 layers; random weights from
  tests/bert_oracle.py - the real all-MiniLM-L6-v2 weights are not needed for a timing) in eval mode, ``enc(ids)[0]`` on a
  NEW id tensor every iteration; (B, T) = (1, 12), (8, 20), (64, 20).  ``perf_counter`` around the call = host enqueue time
  (the device is idle before, nothing waits inside), HIP events around it = stream time.  Median of ``--iters`` after
  ``--warm``; ``--rounds`` repeats the off / on pair: the spread between two runs of one leg is the noise the rule for the
  default is read against;
* ``--arch roberta`` / ``mpnet``: a ``RobertaModel`` / ``MPNetModel`` of the roberta-base / all-mpnet-base-v2 shape (hidden
  768, 12 heads, intermediate 3072, 12 layers, 514 positions; random weights from tests/lm_variants_oracle.py), ids with
  pads in them, the same three (B, T) and the same two legs (``GNNRAG_HIP_LM=0`` / ``=1``); no per-kernel split;
* the per-kernel split of the HIP leg (switch on only): 20 calls captured into one graph and replayed - the whole encode,
  the embedding LayerNorm alone (L = 0), one layer's attention and its four dense products alone; what remains per layer is
  the two LayerNorms and the GELU;
* a whole evaluation forward of a ``BERTInstruction`` ReaRev model is NOT measured here: the reference's ``--lm sbert``
  loader tokenises its data with the hub's tokenizer, which cannot be built offline (recorded as unmeasured).

``--train``: the same encoder in TRAINING mode at transformers' dropout 0.1, as ``Trainer_KBQA`` runs a frozen LM:
``GNNRAG_HIP_LM=1`` in both legs, ``GNNRAG_HIP_LM_TRAIN`` off (transformers' own forward) and on (``draw_keep`` and
``gnnrag_bert_encode_train``), each in a process of its own; the same shapes, host enqueue and stream time; no per-kernel
split.  The draws differ between the legs (and between iterations), so there is no checksum to compare.

``--splitk``: the inference encode with ``GNNRAG_HIP_LM=1`` in both legs and ``GNNRAG_HIP_LM_SPLITK`` off (the encode as it
has always been) and on (``gnnrag_bert_encode_splitk``), each in a process of its own; the same shapes, host enqueue and
stream time.  The on leg lifts ``SPLITK_MAX_ROWS`` so that every shape is measured on the new path: that bound is what the
numbers decide.  ``--splitk --kernel``: device time of the four dense products of a layer at the
MiniLM and the 768-wide shape, 20 calls per graph - ``ops.linear`` (the product alone; its GELU or LayerNorm is one more
launch in the encode) against ``ops.linear_splitk`` (the product, the reduce and the epilogue) at the library's ``splits``,
and at (1, 12) a sweep over forced ``splits`` with the bytes of W over the time beside it.

``--finetune``: forward + backward of the UNFROZEN encoder alone (the reference's ``--lm_frozen 0``) in training mode at
transformers' dropout 0.1: ``out = enc(ids)[0]; out.backward(g)`` with every parameter requiring grad and the gradients
cleared before each iteration, ``GNNRAG_HIP_LM=1`` in both legs and ``GNNRAG_HIP_LM_FINETUNE`` off (transformers and torch
autograd) and on (transformers' embedding stage, the layers on ``gnnrag_bert_layers_forward_save`` /
``gnnrag_bert_layers_backward``), each in a process of its own; the same shapes, host enqueue and stream time of the pair.
``--finetune --full`` (``--arch bert|roberta|mpnet``): ``GNNRAG_HIP_LM_FINETUNE=1`` in both legs and
``GNNRAG_HIP_LM_FINETUNE_FULL`` off (the path above; for MPNet transformers' own forward and backward) and on (the embedding
stage on ``gnnrag_bert_embed_forward_save`` / ``_backward`` as well, MPNet's layers with its relative bias), written to
``profiles/bert_encoder_finetune_full_time.jsonl``.

``--kernel``: ``gnnrag_bert_attention`` alone, 20 calls per graph, per library given in ``--libs`` as ``label=path``
(``GNNRAG_LIB``; empty path = the built library): how the workgroup size (``-DGNNRAG_BERT_ATT_THREADS``,
``build.build_variant``) was chosen."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 12), (8, 20), (64, 20)]
L, VOCAB, MAX_POS = 6, 30522, 512
BASE = dict(H=768, heads=12, I=3072)               # roberta-base, all-mpnet-base-v2: 12 layers, 514 positions
ARCHS = {"bert": "BertModel", "roberta": "RobertaModel", "mpnet": "MPNetModel"}
BASE_L, BASE_VOCAB, BASE_MAX_POS = 12, {"roberta": 50265, "mpnet": 30527}, 514
TAG = "GNNRAG_BERT "
CALLS = 20


def _median(xs):
    xs = sorted(xs)
    n = len(xs)
    return xs[n // 2] if n % 2 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])


def _measure(torch, fn, inputs, warm):
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


def _graph_us(torch, fn, a):
    """Device time of one fn() call in microseconds: CALLS calls in one graph, replayed."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            fn()
    ms = []
    for it in range(a.warm + a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        if it >= a.warm:
            ms.append(e0.elapsed_time(e1) / CALLS)
    return _median(ms) * 1e3


def _setup():
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import torch
    import gnnrag_amd  # noqa: F401
    import bert_oracle as bo
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_bert_encoder.py needs a GPU")
    return torch, bo, torch.device("cuda", 0)


class _Holder:
    def __init__(self, enc):
        self.node_encoder = enc


def child_encode(a):
    torch, bo, dev = _setup()
    import numpy as np
    from gnnrag_amd import ops
    from gnnrag_amd.modules.question_encoding.lm_encoder import enabled, patch_lm_encoder, train_enabled
    on = train_enabled() if a.train else enabled(ARCHS[a.arch])
    if a.splitk:
        from gnnrag_amd.modules.question_encoding import lm_encoder
        on = lm_encoder.splitk_enabled()
        lm_encoder.SPLITK_MAX_ROWS = 1 << 30    # measure every shape on the new path: the bound is read off these numbers
    if a.arch == "bert":
        shape, n_layers, vocab = bo.MINILM, L, VOCAB
        m32 = bo.make_model(bo.config(L=L, vocab=VOCAB, max_pos=MAX_POS, **bo.MINILM), seed=1)[0]
    else:
        import lm_variants_oracle as lo
        shape, n_layers, vocab = BASE, BASE_L, BASE_VOCAB[a.arch]
        model = lo.model_class(a.arch)(lo.config(a.arch, L=BASE_L, vocab=vocab, max_pos=BASE_MAX_POS, **BASE))
        rs = np.random.RandomState(1)
        with torch.no_grad():                   # lo.make_model without its float64 copy (125 M parameters)
            for name, p in model.named_parameters():
                w = rs.standard_normal(tuple(p.shape)) * (0.05 if p.dim() >= 2 else 0.1)
                p.copy_(torch.from_numpy((1.0 + w if name.endswith("LayerNorm.weight") else w).astype(np.float32)))
        m32 = model
    enc = m32.to(dev).train(a.train)
    for p in enc.parameters():
        p.requires_grad_(False)
    patch_lm_encoder(_Holder(enc))
    patch = enc._gnnrag_lm_patch
    for B, T in SHAPES:
        ids0 = np.random.RandomState(B).randint(0 if a.arch == "bert" else 2, vocab, (B, T))
        if a.arch != "bert":
            ids0[1::2, T // 2:] = 1             # every second question padded from the middle (pad id 1)
        ids0 = torch.from_numpy(ids0).long().to(dev)
        ids = [ids0.clone() for _ in range(a.warm + a.iters)]
        out = []

        def encode(x):
            with torch.no_grad():
                out[:] = [enc(x)[0]]

        before, before_train, before_splitk = patch.hip_calls, patch.hip_train_calls, patch.hip_splitk_calls
        host, ev, host_min, ev_min = _measure(torch, encode, ids, a.warm)
        rec = {"what": "encode_train" if a.train else "encode_splitk" if a.splitk else "encode", "arch": a.arch, "switch": "on" if on else "off", "B": B, "T": T, "L": n_layers,
               "H": shape["H"], "I": shape["I"],
               "host_ms": host, "event_ms": ev, "host_ms_min": host_min, "event_ms_min": ev_min, "iters": a.iters,
               "warm": a.warm, "hip_calls_per_encode": (patch.hip_calls - before) / len(ids),
               "checksum": float(out[0].double().square().sum()), "device": torch.cuda.get_device_name(0)}
        if a.splitk:
            rec["hip_splitk_calls_per_encode"] = (patch.hip_splitk_calls - before_splitk) / len(ids)
        if a.train:
            rec["dropout"] = float(enc.config.hidden_dropout_prob)
            rec["hip_train_calls_per_encode"] = (patch.hip_train_calls - before_train) / len(ids)
        print(TAG + json.dumps(rec), flush=True)
        if not on or a.arch != "bert" or a.train or a.splitk:
            continue
        # the split of the HIP leg
        P = bo.layer_params(enc)
        layers = patch.layers()
        top = (P["word_emb"], P["pos_emb"], P["type_emb"], P["ln_g"], P["ln_b"], P["eps"])
        full = _graph_us(torch, lambda: ops.bert_encode(ids0, *top, layers, 12, I=1536), a)
        emb = _graph_us(torch, lambda: ops.bert_encode(ids0, *top, [], 12, I=1536), a)
        lay, M = layers[0], B * T
        x = torch.randn(M, 384, device=dev)
        f = torch.randn(M, 1536, device=dev)
        qkv = torch.randn(M, 1152, device=dev)
        split = {"qkv": _graph_us(torch, lambda: ops.linear(x, lay["W_qkv"], lay["b_qkv"]), a),
                 "attention": _graph_us(torch, lambda: ops.bert_attention(qkv, B, T, 12, 32), a),
                 "out_proj": _graph_us(torch, lambda: ops.linear(x, lay["W_o"], lay["b_o"], add=x), a),
                 "ffn_in": _graph_us(torch, lambda: ops.linear(x, lay["W_i"], lay["b_i"]), a),
                 "ffn_out": _graph_us(torch, lambda: ops.linear(f, lay["W_f"], lay["b_f"], add=x), a)}
        split["two_layernorms_and_gelu"] = (full - emb) / L - sum(split.values())
        rec = {"what": "split", "B": B, "T": T, "L": L, "encode_us": full, "embed_ln_us": emb,
               "per_layer_us": split, "calls_per_graph": CALLS, "iters": a.iters,
               "device": torch.cuda.get_device_name(0)}
        print(TAG + json.dumps(rec), flush=True)
    print(TAG + json.dumps({"what": "forward", "unmeasured": "a BERTInstruction ReaRev forward needs the hub's tokenizer "
                            "in the reference's data loader; it cannot be built offline"}), flush=True)


def child_finetune(a):
    torch, bo, dev = _setup()
    import numpy as np
    from gnnrag_amd.modules.question_encoding.lm_encoder import finetune_enabled, finetune_full_enabled, patch_lm_encoder
    on, full = finetune_enabled(), finetune_full_enabled()
    if a.arch == "bert":
        shape, n_layers, vocab = bo.MINILM, L, VOCAB
        enc = bo.make_model(bo.config(L=L, vocab=VOCAB, max_pos=MAX_POS, **bo.MINILM), seed=1)[0]
    else:
        import lm_variants_oracle as lo
        shape, n_layers, vocab = BASE, BASE_L, BASE_VOCAB[a.arch]
        enc = lo.model_class(a.arch)(lo.config(a.arch, L=BASE_L, vocab=vocab, max_pos=BASE_MAX_POS, **BASE))
    enc = enc.to(dev).train()
    patch_lm_encoder(_Holder(enc))
    patch = enc._gnnrag_lm_patch
    for B, T in SHAPES:
        ids0 = np.random.RandomState(B).randint(0 if a.arch == "bert" else 2, vocab, (B, T))
        if a.arch != "bert":
            ids0[1::2, T // 2:] = 1             # every second question padded from the middle (pad id 1)
        ids0 = torch.from_numpy(ids0).long().to(dev)
        g = torch.randn(B, T, shape["H"], device=dev)
        before, before_full = patch.hip_finetune_calls, patch.hip_finetune_full_calls
        host, ev = [], []
        for it in range(a.warm + a.iters):
            x = ids0.clone()
            enc.zero_grad(set_to_none=True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            enc(x)[0].backward(g)
            t1 = time.perf_counter()
            e1.record()
            e1.synchronize()
            if it >= a.warm:
                host.append((t1 - t0) * 1e3)
                ev.append(e0.elapsed_time(e1))
        rec = {"what": "finetune_fwd_bwd", "arch": a.arch, "switch": "on" if on else "off", "B": B, "T": T, "L": n_layers,
               "H": shape["H"], "I": shape["I"], "host_ms": _median(host), "event_ms": _median(ev), "host_ms_min": min(host),
               "event_ms_min": min(ev), "iters": a.iters, "warm": a.warm, "dropout": float(enc.config.hidden_dropout_prob),
               "hip_finetune_calls_per_encode": (patch.hip_finetune_calls - before) / (a.warm + a.iters),
               "full": "on" if full else "off",
               "hip_finetune_full_calls_per_encode": (patch.hip_finetune_full_calls - before_full) / (a.warm + a.iters),
               "device": torch.cuda.get_device_name(0)}
        print(TAG + json.dumps(rec), flush=True)


def child_kernel(a):
    torch, bo, dev = _setup()
    from gnnrag_amd import ops
    for B, T in SHAPES + [(64, 128)]:
        for heads, dh in ((12, 32), (12, 64)):
            qkv = torch.randn(B * T, 3 * heads * dh, device=dev)
            out = []
            us = _graph_us(torch, lambda: out.__setitem__(slice(None), [ops.bert_attention(qkv, B, T, heads, dh)]), a)
            rec = {"what": "kernel", "threads": a.label, "B": B, "T": T, "heads": heads, "dh": dh, "us_per_call": us,
                   "calls_per_graph": CALLS, "iters": a.iters, "checksum": float(out[0].double().sum()),
                   "device": torch.cuda.get_device_name(0)}
            print(TAG + json.dumps(rec), flush=True)


SWEEP = (1, 2, 4, 8, 16, 32, 64, 128)


def child_splitk_kernel(a):
    """The four products of a layer: the old form (``ops.linear``) against the split-K form, and the sweep at (1, 12)."""
    torch, bo, dev = _setup()
    from gnnrag_amd import _lib, ops
    name = torch.cuda.get_device_name(0)
    for shape_name, shp in (("minilm", bo.MINILM), ("base", BASE)):
        H, I = shp["H"], shp["I"]
        W = {"qkv": torch.randn(3 * H, H, device=dev) * 0.05, "out_proj": torch.randn(H, H, device=dev) * 0.05,
             "ffn_in": torch.randn(I, H, device=dev) * 0.05, "ffn_out": torch.randn(H, I, device=dev) * 0.05}
        epi = {"qkv": "bias", "out_proj": "add_ln", "ffn_in": "gelu", "ffn_out": "add_ln"}
        g, b = torch.ones(H, device=dev), torch.zeros(H, device=dev)
        for B, T in SHAPES:
            M = B * T
            res = torch.randn(M, H, device=dev)
            for prod, w in W.items():
                Nout, K = w.shape
                x = torch.randn(M, K, device=dev)
                bias = torch.randn(Nout, device=dev) * 0.1
                ln = epi[prod] == "add_ln"
                kw = dict(epi=epi[prod], add=res, ln=(g, b, 1e-12)) if ln else dict(epi=epi[prod])
                old = _graph_us(torch, lambda: ops.linear(x, w, bias, add=res if ln else None), a)
                plan = ops.linear_splitk_plan(M, K, Nout)
                new = _graph_us(torch, lambda: ops.linear_splitk(x, w, bias, **kw), a)
                rec = {"what": "splitk_product", "shape": shape_name, "product": prod, "B": B, "T": T, "K": K, "Nout": Nout,
                       "epilogue": epi[prod], "linear_us": old, "splitk_us": new, "splits": plan.splits,
                       "k_chunk": plan.k_chunk, "calls_per_graph": CALLS, "iters": a.iters, "device": name}
                if M <= 16:
                    rec["w_bytes"] = 4 * K * Nout
                    rec["linear_w_tb_s"], rec["splitk_w_tb_s"] = 4e-6 * K * Nout / old, 4e-6 * K * Nout / new
                print(TAG + json.dumps(rec), flush=True)
                if (B, T) != SHAPES[0]:
                    continue
                sweep = {}
                for s in SWEEP:
                    try:
                        ops.linear_splitk_plan(M, K, Nout, s)
                    except _lib.GnnragError:
                        continue                # above K / 4, or a value that would leave an empty chunk
                    sweep[str(s)] = _graph_us(torch, lambda: ops.linear_splitk(x, w, bias, splits=s, **kw), a)
                print(TAG + json.dumps({"what": "splitk_sweep", "shape": shape_name, "product": prod, "B": B, "T": T, "K": K,
                                        "Nout": Nout, "us_by_splits": sweep, "rule_splits": plan.splits, "rule_us": new,
                                        "w_bytes": 4 * K * Nout, "calls_per_graph": CALLS, "iters": a.iters,
                                        "device": name}), flush=True)


def _spawn(argv, env_extra, lines, limit):
    """A fresh child process under its own time limit (nothing replaces the program of a process that holds the GPU)."""
    env = dict(os.environ)
    env.update(env_extra)
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + argv, env=env,
                       capture_output=True, text=True)
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
    ap.add_argument("--arch", choices=sorted(ARCHS), default="bert")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--train", action="store_true", help="training mode at dropout 0.1: GNNRAG_HIP_LM_TRAIN off / on")
    ap.add_argument("--splitk", action="store_true", help="inference: GNNRAG_HIP_LM_SPLITK off / on; with --kernel the products")
    ap.add_argument("--finetune", action="store_true",
                    help="unfrozen, training mode, forward + backward: GNNRAG_HIP_LM_FINETUNE off / on")
    ap.add_argument("--full", action="store_true",
                    help="with --finetune: GNNRAG_HIP_LM_FINETUNE on in both legs, GNNRAG_HIP_LM_FINETUNE_FULL off / on")
    ap.add_argument("--libs", default="256=")
    ap.add_argument("--limit", type=int, default=240, help="seconds one child process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", choices=["encode", "kernel", "splitk_kernel", "finetune"])
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.child:
        return {"encode": child_encode, "kernel": child_kernel, "splitk_kernel": child_splitk_kernel,
                "finetune": child_finetune}[a.child](a)
    if a.finetune and a.arch == "mpnet" and not a.full:
        raise SystemExit("--finetune: MPNetModel keeps transformers' forward in both legs, there is nothing to compare "
                         "(--finetune --full compares it)")
    if a.out is None:
        a.out = os.path.join(REPO, "profiles", "bert_encoder_finetune_full_time.jsonl" if a.finetune and a.full else
                             "bert_encoder_finetune_time.jsonl" if a.finetune else
                             "bert_encoder_splitk_time.jsonl" if a.splitk else "bert_encoder_time.jsonl")
    common = (["--iters", str(a.iters), "--warm", str(a.warm), "--arch", a.arch] + (["--train"] if a.train else []) +
              (["--splitk"] if a.splitk else []))
    lines = []
    if a.finetune:
        for rnd in range(a.rounds):
            for switch in ("0", "1"):
                before = len(lines)
                env = {"GNNRAG_HIP_LM": "1", "GNNRAG_HIP_LM_FINETUNE": switch, "GNNRAG_HIP_LM_FINETUNE_FULL": "0"}
                if a.full:      # GNNRAG_HIP_LM_FINETUNE on in both legs: the off leg is the path without the new switch
                    env.update({"GNNRAG_HIP_LM_FINETUNE": "1", "GNNRAG_HIP_LM_FINETUNE_FULL": switch})
                _spawn(["--child", "finetune"] + common, env, lines, a.limit)
                for rec in lines[before:]:
                    rec["round"] = rnd
    elif a.splitk and a.kernel:
        _spawn(["--child", "splitk_kernel"] + common, {}, lines, a.limit)
    elif a.splitk:
        for rnd in range(a.rounds):
            for switch in ("0", "1"):
                before = len(lines)
                _spawn(["--child", "encode"] + common, {"GNNRAG_HIP_LM": "1", "GNNRAG_HIP_LM_SPLITK": switch}, lines, a.limit)
                for rec in lines[before:]:
                    rec["round"] = rnd
                    rec["splitk"] = "on" if switch == "1" else "off"
    elif a.kernel:
        for spec in a.libs.split(","):
            label, _, path = spec.partition("=")
            env = {"GNNRAG_LIB": os.path.abspath(os.path.join(REPO, path))} if path else {}
            _spawn(["--child", "kernel", "--label", label] + common, env, lines, a.limit)
    else:
        for rnd in range(a.rounds):
            for switch in ("0", "1"):
                before = len(lines)
                env = {"GNNRAG_HIP_LM": "1", "GNNRAG_HIP_LM_TRAIN": switch} if a.train else {"GNNRAG_HIP_LM": switch}
                _spawn(["--child", "encode"] + common, env, lines, a.limit)
                for rec in lines[before:]:
                    rec["round"] = rnd
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
