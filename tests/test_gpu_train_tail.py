"""gnnrag_kl_loss_train / gnnrag_kl_loss_backward / gnnrag_train_metrics on the MI355X against the float64 loss oracle and the
plain-Python restatement of the metrics (tests/train_tail_oracle.py), through ``ops``, ``autograd.KLLossFn`` and
``modules.train_tail.patch_loss_metrics`` with ``GNNRAG_HIP_LOSS_METRICS=1``.

Bounds: loss within 2e-5 of |loss| and d_pred within 2e-5 of its largest entry (the project's bound for every fp32 training
entry point); d_pred exactly 0 where teacher == 0 or label_valid == 0; argmax, H@1, F1 (as fp32 bits) and the four counts
EQUAL to the oracle.  The shapes cover the wave (64), workgroup (1024) and power-of-two boundaries and the raised LDS cap
(16384); question b of a case is built around corner (seed + b) % 9 (``train_tail_oracle.case``), and the small shapes run
every corner."""
import functools
import os

import numpy as np
import pytest
import torch

import train_tail_oracle as to

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_KERNEL = 2e-5
SHAPES = [(1, 1), (2, 2), (2, 3), (3, 64), (2, 65), (3, 1023), (2, 1024), (2, 1025), (3, 2050), (1, 16384)]


def _seeds(B, N):
    return range(to.KINDS) if N <= 65 else (range(0, to.KINDS, 3) if N < 16384 else (6, 8))


def _eps(seed):
    return 0.95 if seed % 2 == 0 else 0.3


@functools.lru_cache(maxsize=None)
def _reference(B, N, seed):
    """(case, loss oracle, metric oracle): computed once, shared, never modified."""
    c = to.case(B, N, seed, _eps(seed))
    for v in c.values():
        if isinstance(v, np.ndarray) and v.ndim:
            v.setflags(write=False)
    return c, to.loss_and_grad(c["pred"], c["teacher"], c["label_valid"], c["g"]), \
        to.metrics(c["pred"], c["answer"], c["seed"], c["local_entity"], c["pad_id"], c["eps"])


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _tensors(dev, c):
    t = {k: torch.from_numpy(np.array(v)).to(dev) for k, v in c.items() if isinstance(v, np.ndarray) and v.ndim}
    t["g"] = torch.tensor([float(c["g"])], dtype=torch.float32, device=dev)
    return t


def _bits(*ts):
    return [t.cpu().numpy().tobytes() for t in ts]


@pytest.mark.parametrize("B,N", SHAPES)
def test_loss_and_backward_against_the_oracle(dev, B, N):
    from gnnrag_amd import ops
    worst = [0.0, 0.0]
    for seed in _seeds(B, N):
        c, (loss64, d64, len64, _), _ = _reference(B, N, seed)
        t = _tensors(dev, c)
        loss, reserve = ops.kl_loss_train(t["pred"], t["teacher"], t["label_valid"])
        d = ops.kl_loss_backward(t["g"], t["pred"], t["teacher"], t["label_valid"], reserve)
        assert tuple(loss.shape) == (1,) and tuple(reserve.shape) == (B,) and tuple(d.shape) == (B, N)
        assert np.array_equal(reserve.cpu().numpy().astype(np.float64), len64)      # sums of 0, 0.5, 1, 2: exact in fp32
        e_loss = abs(float(loss.item()) - loss64)
        e_d = float(np.abs(d.cpu().numpy() - d64).max())
        print("(%d,%d) seed %d: loss %.6f err %.3e (%.3e of |loss|)  d_pred err %.3e of %.3e"
              % (B, N, seed, loss64, e_loss, e_loss / max(abs(loss64), 1e-30), e_d, np.abs(d64).max()))
        assert e_loss <= TOL_KERNEL * abs(loss64)
        assert e_d <= TOL_KERNEL * np.abs(d64).max()
        dead = (c["teacher"] == 0) | np.repeat(c["label_valid"] == 0, N, axis=1)
        assert not d.cpu().numpy()[dead].any()
        if loss64:
            worst[0] = max(worst[0], e_loss / abs(loss64))
        if np.abs(d64).max():
            worst[1] = max(worst[1], e_d / np.abs(d64).max())
        loss2, reserve2 = ops.kl_loss_train(t["pred"], t["teacher"], t["label_valid"])
        d2 = ops.kl_loss_backward(t["g"], t["pred"], t["teacher"], t["label_valid"], reserve2)
        assert _bits(loss, reserve, d) == _bits(loss2, reserve2, d2)                  # a second call: the same bits
    print("(%d,%d) maxima: loss %.3e  d_pred %.3e (bound %.0e)" % (B, N, worst[0], worst[1], TOL_KERNEL))


def _metrics(t, c):
    from gnnrag_amd import ops
    return ops.train_metrics(t["pred"], t["answer"], t["seed"], t["local_entity"], c["pad_id"], c["eps"])


@pytest.mark.parametrize("B,N", SHAPES)
def test_metrics_equal_the_oracle(dev, B, N):
    hits = 0
    for seed in _seeds(B, N):
        c, _, want = _reference(B, N, seed)
        t = _tensors(dev, c)
        got = _metrics(t, c)
        pred, h1, f1, cnt = (x.cpu().numpy() for x in got)
        assert pred.dtype == np.int32 and cnt.dtype == np.int32 and h1.dtype == f1.dtype == np.float32
        assert np.array_equal(pred, want["pred"]), (seed, pred, want["pred"])
        assert np.array_equal(cnt, want["cnt"]), (seed, cnt, want["cnt"])
        assert h1.tobytes() == want["h1"].tobytes(), (seed, h1, want["h1"])
        assert f1.tobytes() == want["f1"].tobytes(), (seed, f1, want["f1"])
        assert _bits(*got) == _bits(*_metrics(t, c))                                 # a second call: the same bits
        hits += int(h1.sum())
    print("(%d,%d): %d questions with H@1 = 1, all outputs equal" % (B, N, hits))
    assert hits > 0


@pytest.mark.parametrize("B,N,seed", [(2, 3, 5), (3, 64, 6), (2, 65, 0), (3, 1023, 3), (2, 1024, 7), (3, 2050, 0)])
def test_a_question_alone_and_inside_a_batch(dev, B, N, seed):
    """Metrics and len_b of question b as they are; the loss and d_pred with every other question's label_valid set to 0 in
    the batch, so that the batch's loss is l_b / B and d_pred[b] carries g / B - both one fp32 division away from the
    question alone."""
    from gnnrag_amd import ops
    c, _, _ = _reference(B, N, seed)
    t = _tensors(dev, c)
    full = _metrics(t, c)
    for b in range(B):
        one = {k: (v[b:b + 1].contiguous() if v.dim() == 2 else v) for k, v in t.items()}
        assert _bits(*_metrics(one, c)) == _bits(*(x[b:b + 1] for x in full))
        valid = torch.zeros_like(t["label_valid"])
        valid[b] = t["label_valid"][b]
        loss_b, res_b = ops.kl_loss_train(t["pred"], t["teacher"], valid)
        d_b = ops.kl_loss_backward(t["g"], t["pred"], t["teacher"], valid, res_b)
        loss_1, res_1 = ops.kl_loss_train(one["pred"], one["teacher"], one["label_valid"])
        g_1 = torch.tensor([np.float32(c["g"]) / np.float32(B)], dtype=torch.float32, device=dev)
        d_1 = ops.kl_loss_backward(g_1, one["pred"], one["teacher"], one["label_valid"], res_1)
        assert _bits(res_1) == _bits(res_b[b:b + 1])
        assert (loss_1.cpu().numpy() / np.float32(B)).tobytes() == loss_b.cpu().numpy().tobytes()
        assert _bits(d_1) == _bits(d_b[b:b + 1])
        others = [i for i in range(B) if i != b]
        assert not d_b[others].any()


@pytest.mark.parametrize("B,N", [(2, 1024), (3, 64)])
def test_float4_and_element_forms_agree(dev, B, N):
    """N % 4 == 0: 16-byte aligned bases take the float4 form, bases offset by one float the element form."""
    from gnnrag_amd import ops
    c, _, _ = _reference(B, N, 0)
    t = _tensors(dev, c)

    def shifted(x):
        flat = torch.empty(x.numel() + 1, dtype=x.dtype, device=dev)
        flat[1:].copy_(x.reshape(-1))
        v = flat[1:].view(x.shape)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    loss, reserve = ops.kl_loss_train(t["pred"], t["teacher"], t["label_valid"])
    d = ops.kl_loss_backward(t["g"], t["pred"], t["teacher"], t["label_valid"], reserve)
    assert t["pred"].data_ptr() % 16 == 0 and t["teacher"].data_ptr() % 16 == 0 and d.data_ptr() % 16 == 0
    sp, st = shifted(t["pred"]), shifted(t["teacher"])
    loss_s, reserve_s = ops.kl_loss_train(sp, st, t["label_valid"])
    d_s = ops.kl_loss_backward(t["g"], sp, st, t["label_valid"], reserve_s)
    assert _bits(loss, reserve, d) == _bits(loss_s, reserve_s, d_s)
    # an output offset by one float: straight through the library
    lib, out = ops._lib.load(), torch.full((B * N + 1,), float("nan"), device=dev)
    rc = lib.gnnrag_kl_loss_backward(t["g"].data_ptr(), t["pred"].data_ptr(), t["teacher"].data_ptr(),
                                     t["label_valid"].data_ptr(), reserve.data_ptr(), B, N, out[1:].data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert _bits(out[1:].view(B, N)) == _bits(d) and bool(torch.isnan(out[0]))
    assert _bits(*_metrics({**t, "pred": sp}, c)) == _bits(*_metrics(t, c))


def test_more_slots_than_the_keys_in_lds_are_refused(dev):
    from gnnrag_amd import _lib, ops
    N = 16385
    assert not ops.train_metrics_supported(1, N) and ops.train_metrics_supported(1, N - 1)
    z = torch.zeros(1, N, device=dev)
    with pytest.raises(_lib.GnnragError) as e:
        ops.train_metrics(z, z, z, torch.zeros(1, N, dtype=torch.int64, device=dev), 5, 0.95)
    assert e.value.code == -2


# -- autograd and the module ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "train_tail_ref.npz"))


def _step(model, t, g, teacher=None):
    pred = t["pred"].clone().requires_grad_(True)
    loss = model.calc_loss_label(curr_dist=pred, teacher_dist=t["teacher"] if teacher is None else teacher,
                                 label_valid=t["label_valid"])
    (loss * g).backward()
    h1, f1 = model.get_eval_metric(pred, t["answer"])
    return loss, pred.grad, h1, f1


@pytest.mark.parametrize("tag", list(to.FIXTURE_CASES))
def test_a_patched_model_matches_the_recorded_reference(dev, golden, monkeypatch, tag):
    from gnnrag_amd import ops
    from gnnrag_amd.modules.train_tail import patch_loss_metrics
    r = {k.split(".", 1)[1]: golden[k] for k in golden.files if k.startswith(tag + ".")}
    B, N, seed, eps = to.FIXTURE_CASES[tag]
    c = to.case(B, N, seed, eps)
    t = _tensors(dev, c)
    calls = {"loss": 0, "bwd": 0, "metric": 0}

    def counted(name, key):
        inner = getattr(ops, name)

        def f(*a, **k):
            calls[key] += 1
            return inner(*a, **k)
        monkeypatch.setattr(ops, name, f)

    counted("kl_loss_train", "loss"), counted("kl_loss_backward", "bwd"), counted("train_metrics", "metric")
    model = patch_loss_metrics(to.StandIn(c, dev))
    monkeypatch.setenv("GNNRAG_HIP_LOSS_METRICS", "1")
    loss, grad, h1, f1 = _step(model, t, float(c["g"]))
    assert calls == {"loss": 1, "bwd": 1, "metric": 1} and model.calls == {"loss": 0, "metric": 0}
    assert loss.dim() == 0 and loss.is_cuda and tuple(h1.shape) == tuple(f1.shape) == (B,) and h1.is_cuda and f1.is_cuda
    assert h1.dtype == f1.dtype == torch.float32
    e_loss = abs(float(loss.detach()) - float(r["loss"])) / abs(float(r["loss"]))
    e_d = float(np.abs(grad.cpu().numpy() - r["d_pred"]).max() / np.abs(r["d_pred"]).max())
    print("%s: loss %.3e  d_pred %.3e against the recorded reference" % (tag, e_loss, e_d))
    assert e_loss <= TOL_KERNEL and e_d <= TOL_KERNEL
    assert _bits(h1, f1) == [r["h1"].tobytes(), r["f1"].tobytes()]
    assert [h1.tolist(), f1.tolist()] == [r["h1"].tolist(), r["f1"].tolist()]          # the forward's own .tolist() pair
    with torch.no_grad():                                                            # no graph: the forward alone
        quiet = model.calc_loss_label(curr_dist=t["pred"], teacher_dist=t["teacher"], label_valid=t["label_valid"])
    assert _bits(quiet) == _bits(loss.detach()) and calls["loss"] == 2 and calls["bwd"] == 1
    # what stays on the reference's method
    before = dict(calls)
    _step(model, t, 1.0, teacher=t["teacher"].clone().requires_grad_(True))          # NSM's backward loss
    assert model.calls == {"loss": 1, "metric": 0} and calls["loss"] == before["loss"] and calls["metric"] == 2
    model.loss_type = "bce"
    _step(model, t, 1.0)
    assert model.calls == {"loss": 2, "metric": 0} and calls["loss"] == before["loss"]
    model.loss_type = "kl"
    monkeypatch.setenv("GNNRAG_HIP_LOSS_METRICS", "0")
    off = _step(model, t, float(c["g"]))
    assert model.calls == {"loss": 3, "metric": 1} and calls["loss"] == before["loss"]
    assert abs(float(off[0].detach()) - float(loss.detach())) <= TOL_KERNEL * abs(float(loss.detach()))
    assert _bits(off[2], off[3]) == _bits(h1, f1)
    monkeypatch.delenv("GNNRAG_HIP_LOSS_METRICS", raising=False)
    _step(model, t, 1.0)
    assert model.calls == {"loss": 4, "metric": 2}
