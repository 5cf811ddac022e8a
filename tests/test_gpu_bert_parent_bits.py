"""Every entry of the LM question encoder, held to the bytes of the library before its host code was folded: before the
inference / training forward and the saving forward shared one layer loop (``bert_layers_run``, csrc/bert_encoder.hip) and
the forward and backward entries one set of argument and keep-plane rules (csrc/bert_host.h).
tests/golden/bert_layers_parent.json names the commit whose library wrote the digests.

Models, ids and masks come from the existing oracles with fixed seeds (tests/bert_dropout_oracle.py,
tests/lm_variants_oracle.py); full-mantissa data, so a launch that is dropped, reordered, given another plane of keep bytes
or another destination changes the bytes.  What the cases cover:

* ``ops.bert_encode`` of BertModel, RobertaModel (positions from the ids), MPNetModel (relative bias) at L = 2, B x T = 3 x 9,
  and of the embedding stage alone (L = 0, 2 x 32), at math fp32 and bf16x3; the split-K encode of the first;
* ``ops.bert_encode_train`` of BertModel and MPNetModel with both masks (p = 0.1 / 0.1), the hidden masks alone and the
  attention masks alone, at both maths;
* ``ops.bert_layers_forward_save`` of BertModel and RobertaModel with masks (0.1 / 0.1) and without, at both maths: one digest
  of ``out`` and one of the WHOLE reserve (every block of every layer: where the loop's destinations point), and
* ``ops.bert_layers_backward`` on each of those reserves: one digest over ``g_x0`` and every gradient of every layer in
  field order.

Every case runs twice and the two runs must agree before they are compared with the golden file.  The digests were recorded
by ``record()`` below, run once with GNNRAG_LIB pointing at the parent commit's build; they are never regenerated from the
code under test.
"""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import bert_dropout_oracle as do
import bert_oracle as bo
import lm_variants_oracle as lo

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bert_layers_parent.json")
MATHS = {"fp32": 0, "bf16x3": 1}
P = 0.1                                           # the dropout probability of every mask that is given

MODELS = {
    "minilm-L2-3x9": ("bert", bo.MINILM, 2, 3, 9),
    "roberta32-L2-3x9": ("roberta", lo.SMALL[32], 2, 3, 9),
    "roberta-L2-3x9": ("roberta", lo.SMALL[32], 2, 3, 9),          # the name the fine-tuning tests give the same model
    "mpnet32-L2-3x9": ("mpnet", lo.SMALL[32], 2, 3, 9),
    "minilm-L0-2x32": ("bert", bo.MINILM, 0, 2, 32),
}
SITES = {"both": (P, P), "hidden-only": (P, None), "attention-only": (None, P), "none": (None, None)}

# case -> (entry, model, masks, math)
CASES = {}
for _m in ("minilm-L2-3x9", "roberta32-L2-3x9", "mpnet32-L2-3x9", "minilm-L0-2x32"):
    for _math in MATHS:
        CASES["encode/%s/%s" % (_m, _math)] = ("encode", _m, "none", _math)
CASES["encode_splitk/minilm-L2-3x9"] = ("splitk", "minilm-L2-3x9", "none", "fp32")
for _m in ("minilm-L2-3x9", "mpnet32-L2-3x9"):
    for _s in ("both", "hidden-only", "attention-only"):
        for _math in MATHS:
            CASES["train/%s/%s/%s" % (_m, _s, _math)] = ("train", _m, _s, _math)
for _m in ("minilm-L2-3x9", "roberta-L2-3x9"):
    for _s in ("both", "none"):
        for _math in MATHS:
            CASES["layers/%s/%s/%s" % (_m, _s, _math)] = ("layers", _m, _s, _math)


@pytest.fixture(scope="module")
def dev():
    pytest.importorskip("transformers")
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=1)
def _golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@functools.lru_cache(maxsize=None)
def _model(name):
    """(fp32 model, ids): built once on the CPU, shared, not modified."""
    arch, shape, L, B, T = MODELS[name]
    if arch == "bert":
        return do.make_bert(shape, L, seed=41)[0], np.random.RandomState(42).randint(0, 64, (B, T))
    return do.make_variant(arch, shape, L, seed=41)[0], lo.ids_with_pads(B, T)              # pad ids present


@functools.lru_cache(maxsize=None)
def _masks(name, sites):
    """The packed keep bytes and the two scales of one (model, sites) pair."""
    _, shape, L, B, T = MODELS[name]
    p_h, p_a = SITES[sites]
    kh, ka = do.pack(do.draw(43, L, B, T, shape["H"], shape["heads"], p_h, p_a), L)
    return kh, ka, (1.0 if p_h is None else do.scale(p_h)), (1.0 if p_a is None else do.scale(p_a))


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def _run_once(case, dev):
    """{what: digest} of one run of the case."""
    from gnnrag_amd import ops
    entry, name, sites, math = CASES[case]
    _, shape, L, B, T = MODELS[name]
    model, ids = _model(name)
    kh, ka, sh, sa = _masks(name, sites)
    math = MATHS[math]
    if entry == "encode":
        return {"out": _sha(lo.encode(dev, model, ids, math=math))}
    if entry == "splitk":
        par = lo.layer_params(model, T)
        on = lambda t: None if t is None else t.detach().to(dev)
        layers = [{k: on(v) for k, v in d.items()} for d in par["layers"]]
        out = ops.bert_encode(torch.from_numpy(ids).long().to(dev), on(par["word_emb"]), on(par["pos_emb"]),
                              on(par["type_emb"]), on(par["ln_g"]), on(par["ln_b"]), par["eps"], layers, par["heads"],
                              I=par["I"], math=math, pad_id=par["pad_id"], rel_bias=on(par["rel_bias"]), splitk=True)
        return {"out": _sha(out)}
    if entry == "train":
        return {"out": _sha(do.encode_train(dev, model, ids, kh, ka, sh, sa, math=math))}
    # the layers: x0 is the embedding stage (plane 0 of the hidden masks), then the saving forward and its backward
    x0 = do.encode_train(dev, model, ids, None if kh is None else kh[:1], None, sh, sa, L=0, math=math)
    par = lo.layer_params(model, T)
    layers = [{k: v.detach().to(dev) for k, v in d.items()} for d in par["layers"]]
    kw = dict(keep_hidden=None if kh is None else torch.from_numpy(kh).to(dev), scale_hidden=sh,
              keep_att=None if ka is None else torch.from_numpy(ka).to(dev), scale_att=sa)
    out, reserve = ops.bert_layers_forward_save(x0, layers, par["heads"], par["eps"], B, T, math, **kw)
    assert reserve.numel() == L * B * T * (8 * shape["H"] + shape["I"]) * 4
    g_out = torch.from_numpy(np.random.RandomState(44).standard_normal((B, T, shape["H"])).astype(np.float32)).to(dev)
    g_x0, grads = ops.bert_layers_backward(g_out, layers, par["heads"], par["eps"], B, T, reserve, **kw)
    return {"out": _sha(out), "reserve": _sha(reserve),
            "backward": _sha(g_x0, *[grads[l][f] for l in range(L) for f in ops.BERT_GRAD_FIELDS])}


def run_case(case, dev):
    return [_run_once(case, dev) for _ in range(2)]


@pytest.mark.parametrize("case", list(CASES))
def test_encoder_bytes_are_the_parents(dev, case):
    first, again = run_case(case, dev)
    assert first == again, case + ": two calls differ"
    assert first == _golden()["digests"][case], case + ": not the bytes the parent's library wrote"


def record(path, commit):
    """Writes the golden file; run once with GNNRAG_LIB naming the build of ``commit``."""
    dev = torch.device("cuda", 0)
    out = {"parent_commit": commit, "device": torch.cuda.get_device_name(0), "digests": {}}
    for case in CASES:
        first, again = run_case(case, dev)
        assert first == again, case
        out["digests"][case] = first
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
