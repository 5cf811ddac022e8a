"""gnnrag_kl_loss_train, gnnrag_kl_loss_backward and gnnrag_train_metrics in guarded buffers (tests/guarded.py): every buffer
the binding allocates (``ops._buf``: loss, reserve, the workspace, d_pred, the four metric outputs) and every input is an
exact-sized view between two 64 KiB guards; the calls run on a non-default stream with the buffers pre-filled with 0x00, with
the leftovers of a call on other inputs and with 0xFF.  All guards and inputs must hold their bytes, and the three results
and the unguarded one must be the same bits: ``d_pred`` in particular is fully written and nothing is accumulated into what
a buffer held."""
import re

import numpy as np
import pytest
import torch

import guarded
import train_tail_oracle as to
from guarded import FILL_LEFTOVERS, FILL_ONES, FILL_ZERO

pytestmark = pytest.mark.gpu
TOL_KERNEL = 2e-5


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _tensors(dev, c):
    t = {k: torch.from_numpy(v).to(dev) for k, v in c.items() if isinstance(v, np.ndarray) and v.ndim}
    t["g"] = torch.tensor([float(c["g"])], dtype=torch.float32, device=dev)
    return t


def _wrap(g, t):
    return {k: g.wrap(v, "input " + k) for k, v in t.items()}


def _call(t, c, stream):
    """Loss, backward and metrics on ``stream``; everything they return as one flat list of host tensors."""
    from gnnrag_amd import ops
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        loss, reserve = ops.kl_loss_train(t["pred"], t["teacher"], t["label_valid"])
        d = ops.kl_loss_backward(t["g"], t["pred"], t["teacher"], t["label_valid"], reserve)
        m = ops.train_metrics(t["pred"], t["answer"], t["seed"], t["local_entity"], c["pad_id"], c["eps"])
    stream.synchronize()
    return [o.cpu() for o in (loss, reserve, d) + tuple(m)]


# N % 4 != 0 (the element form of the backward; keys padded to a power of two); N % 4 == 0 (float4 accesses)
@pytest.mark.parametrize("B,N", [(3, 67), (2, 1024)])
def test_loss_backward_and_metrics_guarded(dev, monkeypatch, B, N):
    from gnnrag_amd import ops
    c, other = to.case(B, N, seed=6), to.case(B, N, seed=2)
    plain_in, other_in = _tensors(dev, c), _tensors(dev, other)
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.default_stream().cuda_stream
    plain = _call(plain_in, c, side)

    g = guarded.Guard(dev)
    guarded.install(monkeypatch, g)
    assert ops._buf == g.buf
    runs = []
    for fill, inp, cc in ((FILL_ZERO, plain_in, c), (FILL_ZERO, other_in, other), (FILL_LEFTOVERS, plain_in, c),
                          (FILL_ONES, plain_in, c)):
        g.fill = fill
        hits = g.leftover_hits
        out = _call(_wrap(g, inp), cc, side)
        if fill == FILL_LEFTOVERS:
            assert g.leftover_hits > hits
        g.check("body fill %r%s" % (fill, "" if inp is plain_in else " (other inputs)"))
        if inp is plain_in:
            runs.append(out)
    fwd, bwd, met = "kl_loss_train: ", "kl_loss_backward: ", "train_metrics: "
    want_sizes = {fwd + "loss": 4, fwd + "reserve": B * 4, bwd + "d_pred": B * N * 4, met + "pred": B * 4, met + "h1": B * 4,
                  met + "f1": B * 4, met + "counts": B * 16}
    assert set(g.sizes) == set(want_sizes) | {fwd + "workspace"}
    for role, size in want_sizes.items():
        assert g.sizes[role] == size, role
    assert g.sizes[fwd + "workspace"] == ops._lib.load().gnnrag_kl_loss_workspace_bytes(B) >= B * 4
    for out in runs:
        assert len(out) == len(plain)
        for i, (got, want) in enumerate(zip(out, plain)):
            assert got.shape == want.shape and got.numpy().tobytes() == want.numpy().tobytes(), "output %d" % i
    # and the guarded results are right
    loss64, d64, _, _ = to.loss_and_grad(c["pred"], c["teacher"], c["label_valid"], c["g"])
    want = to.metrics(c["pred"], c["answer"], c["seed"], c["local_entity"], c["pad_id"], c["eps"])
    loss, _, d, pred, h1, f1, cnt = runs[-1]
    assert abs(float(loss) - loss64) <= TOL_KERNEL * abs(loss64)
    assert np.abs(d.numpy() - d64).max() <= TOL_KERNEL * np.abs(d64).max()
    assert np.array_equal(pred.numpy(), want["pred"]) and np.array_equal(cnt.numpy(), want["cnt"])
    assert h1.numpy().tobytes() == want["h1"].tobytes() and f1.numpy().tobytes() == want["f1"].tobytes()
    g.release()


def test_a_workspace_stated_four_bytes_short_is_refused_and_nothing_is_written(dev, monkeypatch):
    from gnnrag_amd import _lib, ops
    t = _tensors(dev, to.case(3, 67, seed=6))
    g = guarded.Guard(dev, fill=FILL_ONES)
    guarded.install(monkeypatch, g)
    g.short = {"kl_loss_train: workspace": 4}
    first = len(g.blocks)
    with pytest.raises(_lib.GnnragError) as e:
        ops.kl_loss_train(t["pred"], t["teacher"], t["label_valid"])
    assert int(re.search(r"failed \((-?\d+)\)", str(e.value)).group(1)) == -3
    g.check("workspace four bytes short")
    assert len(g.blocks) - first == 3                  # loss, reserve, workspace
    for b in g.blocks[first:]:                         # nothing was launched: every buffer still holds its 0xFF fill
        assert bool((b.raw[g.G: g.G + b.nbytes] == 0xFF).all()), b.role
    g.short = {}
    ops.kl_loss_train(t["pred"], t["teacher"], t["label_valid"])
    g.check("stated size again")
    g.release()
