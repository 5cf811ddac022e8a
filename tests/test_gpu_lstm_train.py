"""The training form of the LSTM on the MI355X: gnnrag_lstm_forward_train / gnnrag_lstm_backward, autograd.LstmFn and
HipLSTM under autograd.

Truth: torch.nn.LSTM in float64 on the CPU with the same parameters, random g_out / g_hn / g_cn through
``(out * g_out).sum() + (h_n * g_hn).sum() + (c_n * g_cn).sum()``.  Tolerance: the project's kernel rule
(test_gpu_backward._close, TOL_KERNEL): per gradient tensor ``|diff| <= 2e-5 * max(max|want|, 1e-6)``.  torch's own fp32
CPU backward stays within 2.2e-6 of that scale on every shape below, so the bound leaves about 9x over an fp32 reference.

The round after an optimiser step is held to TOL_MODULE (3e-4) instead: there the device and the truth no longer start
from the same weights - the device's weights carry lr times the first round's (in-tolerance) gradient error, a relative
weight perturbation of up to lr * 2e-5 * max|g| / |w| (about 1e-5 at lr = 0.002, max|g| near 20 in the float64 truth -
sums of 288 products of a unit normal and a gate gradient - and |w| <= 1/sqrt(200) = 0.07), and the gradient's
sensitivity to the weights multiplies it - which the kernel rule, made for equal inputs, does not allow for.  Plain SGD on purpose:
Adam's first step is lr * g / (|g| + eps), which turns a last-bit difference of a near-zero gradient into a weight
difference of up to 2 lr, so fp32 and float64 runs are not comparable through it."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import guarded
from guarded import FILL_ONES, FILL_ZERO

pytestmark = pytest.mark.gpu

TOL_KERNEL = 2e-5          # test_gpu_backward.py
TOL_MODULE = 3e-4
E_WORKSPACE = -3


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


@pytest.fixture
def g(dev, monkeypatch):
    from gnnrag_amd import ops
    guard = guarded.Guard(dev)
    guard.plain = ops._buf
    guarded.install(monkeypatch, guard)
    yield guard
    guard.release()


def _close(got, want, tol, msg, floor=1e-6):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    want = want.detach().numpy() if isinstance(want, torch.Tensor) else want
    assert got.shape == want.shape, msg
    err, scale = np.abs(got - want).max(), max(np.abs(want).max(), floor)
    print("%-28s max|diff| %.3e  scale %.3e  ratio %.3e" % (msg, err, scale, err / scale))
    np.testing.assert_allclose(got, want, rtol=0, atol=tol * scale, err_msg=msg)


# (B, T, E, H, initial states given and requiring grad, bias)
SHAPES = {
    "one_step": (1, 1, 300, 50, False, True),          # no recurrence: dW_hh is exactly zero (the floor of _close)
    "h50_t13": (3, 13, 300, 50, True, True),           # H % 4 != 0, T % 4 != 0 (the forward's token chunk)
    "encoder": (16, 9, 300, 200, False, True),
    "limit": (20, 7, 64, 256, False, True),            # 4 H = 1024 threads
    "r4_ragged": (513, 5, 100, 52, True, True),        # B > 512: four sequences per workgroup, one in the last
    "no_bias": (5, 4, 32, 24, True, False),
    "long": (2, 40, 32, 24, False, True),
}
NAMES = ("dx", "dw_ih", "dw_hh", "db", "dh0", "dc0")


@functools.lru_cache(maxsize=None)
def _case(name):
    """fp32 inputs of a shape and the float64 CPU truth of every gradient (computed once, never changed)."""
    B, T, E, H, states, bias = SHAPES[name]
    torch.manual_seed(1000 + B + 7 * T + H)
    ref = nn.LSTM(E, H, batch_first=True, bias=bias)
    c = {"x": torch.randn(B, T, E), "g_out": torch.randn(B, T, H), "g_hn": torch.randn(B, H), "g_cn": torch.randn(B, H),
         "h0": torch.randn(B, H) if states else None, "c0": torch.randn(B, H) if states else None,
         "w_ih": ref.weight_ih_l0.detach().clone(), "w_hh": ref.weight_hh_l0.detach().clone(),
         "b_ih": ref.bias_ih_l0.detach().clone() if bias else None, "b_hh": ref.bias_hh_l0.detach().clone() if bias else None}
    ref = ref.double()
    x = c["x"].double().requires_grad_(True)
    hx = None
    if states:
        hx = (c["h0"].double()[None].requires_grad_(True), c["c0"].double()[None].requires_grad_(True))
    out, (h_n, c_n) = ref(x, hx)
    ((out * c["g_out"].double()).sum() + (h_n[0] * c["g_hn"].double()).sum() + (c_n[0] * c["g_cn"].double()).sum()).backward()
    want = {"dx": x.grad, "dw_ih": ref.weight_ih_l0.grad, "dw_hh": ref.weight_hh_l0.grad}
    if bias:
        want["db"] = ref.bias_ih_l0.grad
        assert torch.allclose(ref.bias_ih_l0.grad, ref.bias_hh_l0.grad, rtol=0, atol=1e-12)      # one db serves both
    if states:
        want["dh0"], want["dc0"] = hx[0].grad[0], hx[1].grad[0]
    c["want"] = {k: v.detach().numpy().copy() for k, v in want.items()}
    return c


def _to(dev, c, *keys):
    return [None if c[k] is None else c[k].to(dev) for k in keys]


@pytest.mark.parametrize("name", list(SHAPES))
def test_gradients_against_the_float64_module(dev, name):
    from gnnrag_amd import ops
    B, T, E, H, states, bias = SHAPES[name]
    c = _case(name)
    x, w_ih, w_hh, b_ih, b_hh, h0, c0, g_out, g_hn, g_cn = _to(dev, c, "x", "w_ih", "w_hh", "b_ih", "b_hh", "h0", "c0",
                                                               "g_out", "g_hn", "g_cn")
    out, h_n, c_n, reserve = ops.lstm_forward_train(x, w_ih, w_hh, b_ih, b_hh, h0, c0)
    inf = ops.lstm_forward(x, w_ih, w_hh, b_ih, b_hh, h0, c0)
    assert torch.equal(out, inf[0]) and torch.equal(h_n, inf[1]) and torch.equal(c_n, inf[2])
    assert reserve.dtype == torch.uint8 and reserve.numel() == B * T * 5 * H * 4

    def run():
        return ops.lstm_backward(x, w_ih, w_hh, h0, c0, out, reserve, g_out, g_hn, g_cn, need_dx=True, need_db=bias,
                                 need_dh0=states, need_dc0=states)

    got = dict(zip(NAMES, run()))
    for k in NAMES:
        if k in c["want"]:
            _close(got[k], c["want"][k], TOL_KERNEL, "%s %s" % (name, k))
        else:
            assert got[k] is None, k
    if name == "one_step":
        assert not got["dw_hh"].any().item()
    for a, b in zip(got.values(), run()):               # one fixed summation order
        assert (a is None and b is None) or torch.equal(a, b)


def test_null_gradients_and_unwanted_outputs_are_the_full_run_with_zeros(dev, monkeypatch):
    """Through autograd (an output that the loss does not use reaches LstmFn.backward as None and the library as NULL;
    a frozen input gets no dx): bit for bit the explicit call with zero tensors in place of the NULLs."""
    from gnnrag_amd import ops
    from gnnrag_amd.modules.question_encoding.lstm import HipLSTM
    monkeypatch.setenv("GNNRAG_HIP_LSTM_TRAIN", "1")
    name = "h50_t13"
    B, T, E, H, _, _ = SHAPES[name]
    c = _case(name)
    x, w_ih, w_hh, b_ih, b_hh, h0, c0, g_out, g_hn, g_cn = _to(dev, c, "x", "w_ih", "w_hh", "b_ih", "b_hh", "h0", "c0",
                                                               "g_out", "g_hn", "g_cn")
    mod = HipLSTM(E, H, batch_first=True).to(dev).train()
    with torch.no_grad():
        for p, v in zip((mod.weight_ih_l0, mod.weight_hh_l0, mod.bias_ih_l0, mod.bias_hh_l0), (w_ih, w_hh, b_ih, b_hh)):
            p.copy_(v)
    out, _, _, reserve = ops.lstm_forward_train(x, w_ih, w_hh, b_ih, b_hh, h0, c0)
    z_out, z_h = torch.zeros_like(g_out), torch.zeros_like(g_hn)
    combos = {"g_out": (g_out, z_h, z_h), "g_hn": (z_out, g_hn, z_h), "g_cn": (z_out, z_h, g_cn), "no_dx": (g_out, g_hn, g_cn)}
    for tag, (a, b_, c_) in combos.items():
        xi = x.clone().requires_grad_(tag != "no_dx")
        hi, ci = h0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
        mod.zero_grad(set_to_none=True)
        o, (hn, cn) = mod(xi, (hi[None], ci[None]))
        loss = {"g_out": lambda: (o * g_out).sum(), "g_hn": lambda: (hn[0] * g_hn).sum(), "g_cn": lambda: (cn[0] * g_cn).sum(),
                "no_dx": lambda: (o * g_out).sum() + (hn[0] * g_hn).sum() + (cn[0] * g_cn).sum()}[tag]()
        loss.backward()
        full = dict(zip(NAMES, ops.lstm_backward(x, w_ih, w_hh, h0, c0, out, reserve, a, b_, c_, need_dx=True, need_db=True,
                                                 need_dh0=True, need_dc0=True)))
        got = {"dx": xi.grad, "dw_ih": mod.weight_ih_l0.grad, "dw_hh": mod.weight_hh_l0.grad, "db": mod.bias_ih_l0.grad,
               "dh0": hi.grad, "dc0": ci.grad}
        assert (xi.grad is None) == (tag == "no_dx")
        for k in NAMES:
            if got[k] is not None:
                assert torch.equal(got[k], full[k]), (tag, k)
        assert torch.equal(mod.bias_hh_l0.grad, full["db"]), tag
        assert mod.bias_hh_l0.grad.data_ptr() != mod.bias_ih_l0.grad.data_ptr()


def _encoder_pair(dev, seed=5):
    from gnnrag_amd.modules.question_encoding.lstm import HipLSTM
    torch.manual_seed(seed)
    cpu = nn.LSTM(300, 200, batch_first=True)
    gpu = nn.LSTM(300, 200, batch_first=True)
    gpu.load_state_dict(cpu.state_dict())
    hip = HipLSTM.sharing(gpu.to(dev)).train()
    return cpu.double().train(), hip


def _encoder_round(mod, xs, ws, device, dtype):
    """The encoder's pattern (base_encoder.py:74-80): zero [1,B,H] states without grad, two calls inside one graph, out of
    both and h_n of the first in the loss, one backward.  Returns the leaf inputs."""
    B, H = xs[0].shape[0], mod.hidden_size
    zeros = torch.zeros(1, B, H, device=device, dtype=dtype)
    leaves = [x.to(device=device, dtype=dtype).clone().requires_grad_(True) for x in xs]
    w = [t.to(device=device, dtype=dtype) for t in ws]
    o1, (h1, _) = mod(leaves[0], (zeros, zeros))
    o2, _ = mod(leaves[1], (zeros, zeros))
    ((o1 * w[0]).sum() + (h1[0] * w[1]).sum() + (o2 * w[2]).sum()).backward()
    return leaves


def _encoder_data(seed=6):
    torch.manual_seed(seed)
    xs = [torch.randn(16, 9, 300), torch.randn(16, 9, 300)]
    ws = [torch.randn(16, 9, 200), torch.randn(16, 200), torch.randn(16, 9, 200)]
    return xs, ws


def test_the_encoders_pattern_trains_without_the_parent_class(dev, monkeypatch):
    """Two calls of one module inside one graph, both backward passes after both forwards: each needs the reserve of
    ITS forward.  nn.LSTM.forward raises for the duration: the test passes only when training runs on the library."""
    cpu, hip = _encoder_pair(dev)
    xs, ws = _encoder_data()
    want_leaves = _encoder_round(cpu, xs, ws, "cpu", torch.float64)
    monkeypatch.setenv("GNNRAG_HIP_LSTM_TRAIN", "1")

    def refuse(self, *a, **k):
        raise AssertionError("training went to torch.nn.LSTM.forward")

    monkeypatch.setattr(nn.LSTM, "forward", refuse)
    got_leaves = _encoder_round(hip, xs, ws, dev, torch.float32)
    for k, (a, b) in enumerate(zip(got_leaves, want_leaves)):
        _close(a.grad, b.grad, TOL_KERNEL, "encoder dx%d" % k)
    for (n, p), q in zip(hip.named_parameters(), cpu.parameters()):
        _close(p.grad, q.grad, TOL_KERNEL, "encoder " + n)
    # the switch hands training back to the parent class
    monkeypatch.setenv("GNNRAG_HIP_LSTM_TRAIN", "0")
    with pytest.raises(AssertionError, match="went to torch.nn.LSTM.forward"):
        _encoder_round(hip, xs, ws, dev, torch.float32)
    # ... and inference stays on the library either way
    with torch.no_grad():
        hip(xs[0].to(dev))


def test_the_second_round_sees_the_weights_of_the_optimiser_step(dev, monkeypatch):
    """forward/backward, SGD step, forward/backward: the per-module scratch (transposed weights) is refilled by every
    forward.  TOL_MODULE and SGD: see the module docstring."""
    monkeypatch.setenv("GNNRAG_HIP_LSTM_TRAIN", "1")
    cpu, hip = _encoder_pair(dev, seed=8)
    xs, ws = _encoder_data(seed=9)
    opts = [torch.optim.SGD(m.parameters(), lr=0.002) for m in (cpu, hip)]
    first = None
    for rnd in range(2):
        for o in opts:
            o.zero_grad(set_to_none=True)
        want_leaves = _encoder_round(cpu, xs, ws, "cpu", torch.float64)
        got_leaves = _encoder_round(hip, xs, ws, dev, torch.float32)
        tol = TOL_KERNEL if rnd == 0 else TOL_MODULE
        for k, (a, b) in enumerate(zip(got_leaves, want_leaves)):
            _close(a.grad, b.grad, tol, "round %d dx%d" % (rnd, k))
        for (n, p), q in zip(hip.named_parameters(), cpu.parameters()):
            _close(p.grad, q.grad, tol, "round %d %s" % (rnd, n))
        if rnd == 0:
            first = [q.grad.clone() for q in cpu.parameters()]
            for o in opts:
                o.step()
    # the step matters at this tolerance: the truth's own gradients moved by far more than the bound
    for f, q in zip(first, cpu.parameters()):
        assert (f - q.grad).abs().max().item() > 10 * TOL_MODULE * q.grad.abs().max().item()


# -- guarded buffers ------------------------------------------------------------------------------------------------------

def _guarded_call(dev, name):
    from gnnrag_amd import ops
    _, _, _, _, states, bias = SHAPES[name]
    c = _case(name)

    def call(x, w_ih, w_hh, b_ih, b_hh, h0, c0, g_out, g_hn, g_cn):
        out, h_n, c_n, reserve = ops.lstm_forward_train(x, w_ih, w_hh, b_ih, b_hh, h0, c0)
        grads = ops.lstm_backward(x, w_ih, w_hh, h0, c0, out, reserve, g_out, g_hn, g_cn, need_dx=True, need_db=bias,
                                  need_dh0=states, need_dc0=states)
        return [out, h_n, c_n, reserve] + [t for t in grads if t is not None]

    return call, _to(dev, c, "x", "w_ih", "w_hh", "b_ih", "b_hh", "h0", "c0", "g_out", "g_hn", "g_cn")


@pytest.mark.parametrize("name", ["h50_t13", "encoder", "no_bias"])
def test_guarded_exact_sizes_and_no_dependence_on_old_bytes(dev, g, name):
    """Every output, the reserve and both workspaces at exactly their stated sizes between intact guards, inputs
    untouched; the same bits whether the fresh buffers held 0x00 or 0xFF (the reserve included: fully written), and the
    same as the unguarded call."""
    from gnnrag_amd import ops
    call, inputs = _guarded_call(dev, name)
    runs = []
    for fill in (FILL_ZERO, FILL_ONES):
        g.fill = fill
        w = [None if t is None else g.wrap(t, "input %d" % i) for i, t in enumerate(inputs)]
        runs.append([o.detach().cpu().clone() for o in call(*w)])
        g.check("body fill %r" % fill)
    B, T, E, H = SHAPES[name][:4]
    assert g.sizes["lstm_forward_train: reserve"] == B * T * 5 * H * 4
    assert g.sizes["lstm_backward: workspace"] > 256 and g.sizes["lstm_forward_train: workspace"] > 256
    saved, ops._buf = ops._buf, g.plain
    try:
        runs.append([o.detach().cpu().clone() for o in call(*inputs)])
    finally:
        ops._buf = saved
    for r in runs[1:]:
        assert len(r) == len(runs[0])
        for i, (a, b) in enumerate(zip(runs[0], r)):
            assert a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes(), "output %d" % i


def _refused(fn):
    """None when the call was refused with GNNRAG_E_WORKSPACE, else what happened instead."""
    import re
    from gnnrag_amd import _lib
    try:
        fn()
    except _lib.GnnragError as e:
        m = re.search(r"failed \((-?\d+)\)", str(e))
        return None if m and int(m.group(1)) == E_WORKSPACE else str(e)
    return "accepted"


def test_a_sized_buffer_one_byte_short_is_refused_and_nothing_is_written(dev, g):
    from gnnrag_amd import ops
    name = "h50_t13"
    c = _case(name)
    x, w_ih, w_hh, b_ih, b_hh, h0, c0, g_out = _to(dev, c, "x", "w_ih", "w_hh", "b_ih", "b_hh", "h0", "c0", "g_out")
    out, _, _, reserve = ops.lstm_forward_train(x, w_ih, w_hh, b_ih, b_hh, h0, c0)
    g.check("stated sizes")

    def fwd():
        return ops.lstm_forward_train(x, w_ih, w_hh, b_ih, b_hh, h0, c0)

    def bwd(res=reserve):
        return ops.lstm_backward(x, w_ih, w_hh, h0, c0, out, res, g_out, need_dh0=True, need_dc0=True)

    g.fill = FILL_ONES
    cases = [("lstm_forward_train: reserve", fwd), ("lstm_forward_train: workspace", fwd), ("lstm_backward: workspace", bwd),
             (None, lambda: bwd(reserve[:-1]))]
    for role, fn in cases:
        g.short = {role: 1} if role else {}
        first = len(g.blocks)
        assert _refused(fn) is None, role or "lstm_backward: reserve"
        g.check("%s one byte short" % (role or "lstm_backward: reserve"))
        # nothing was launched: every buffer the refused call allocated still holds its 0xFF fill
        for b in g.blocks[first:]:
            assert bool((b.raw[g.G: g.G + b.nbytes] == 0xFF).all()), (role, b.role)
    g.short = {}
    bwd()                                                       # the stated sizes: accepted
    g.check("stated sizes again")
