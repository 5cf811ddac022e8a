"""Guarded-buffer tests of gnnrag_grad_norm / gnnrag_adam_step (tests/guarded.py, as tests/test_gpu_guarded.py uses it): p, g,
m, v, the segment table, out2 and the workspace each sit between two 64 KiB guards; the workspace and out2 start as 0x00,
as the leftovers of a call on other inputs, and as 0xFF; results are bit-identical across the three fills and the
unguarded run; guards, g and the table hold their bytes after every run; one byte less than gnnrag_optim_workspace_bytes is
refused with GNNRAG_E_WORKSPACE; a call on a side stream right after a torch op produced g there gives the same bits.
No test here makes a kernel go out of bounds."""
import re

import numpy as np
import pytest
import torch

import guarded
from guarded import FILL_LEFTOVERS, FILL_ONES, FILL_ZERO

pytestmark = pytest.mark.gpu
E_WORKSPACE = -3
SIZES = [1, 255, 4097, 8193, 1001]          # the last tensor starts one element into its block (4-byte path)
UNALIGNED = 4
MAX_NORM = 1.0


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


def _data(seed):
    rng = np.random.default_rng(seed)
    f = lambda n, s=1.0: (rng.standard_normal(n) * s).astype(np.float32)
    return {"p": [f(n) for n in SIZES], "g": [f(n, 0.05) for n in SIZES], "m": [f(n, 0.01) for n in SIZES],
            "v": [np.abs(f(n, 1e-3)) for n in SIZES]}


def _place(guard, dev, arr, role, i, inp):
    """A device copy of arr: inside guards when a guard is given (g as a wrapped input whose bytes are checked, p / m / v
    as buffers the call may write), tensor UNALIGNED one element into its block."""
    lead = 1 if i == UNALIGNED else 0
    t = torch.zeros(arr.size + lead, device=dev)
    t[lead:].copy_(torch.from_numpy(arr))
    if guard is not None:
        if inp:
            t = guard.wrap(t, role)
        else:
            w = guard.alloc(t.shape, torch.float32, dev, fill=FILL_ONES, role=role)
            w.copy_(t)
            t = w
    t = t[lead:]
    assert t.data_ptr() % 16 == 4 * lead
    return t


def _run(guard, dev, data, produce_g=None):
    """grad_norm + adam_step over the five tensors; returns [out2] + p + m + v."""
    from gnnrag_amd import ops
    t = {k: [_place(guard, dev, a, "%s %d" % (k, i), i, k == "g") for i, a in enumerate(data[k])] for k in "pgmv"}
    if produce_g is not None:
        t["g"] = produce_g(t["g"])
    T = len(SIZES)
    tab = np.zeros(T, dtype=ops.OPTIM_SEG_DTYPE)
    for k in "pgmv":
        tab[k] = [x.data_ptr() for x in t[k]]
    tab["n"] = SIZES
    tab["first_chunk"], n_chunks = ops.optim_chunks(SIZES)
    step = 3
    for i in range(T):
        wd = 0.01 if i % 2 else 0.0
        tab[i]["beta1"], tab[i]["beta2"], tab[i]["om_beta1"], tab[i]["om_beta2"] = 0.9, 0.999, 1 - 0.9, 1 - 0.999
        tab[i]["eps"], tab[i]["weight_decay"] = 1e-8, wd
        tab[i]["step_size"], tab[i]["bc2_sqrt"] = 1e-3 / (1 - 0.9 ** step), (1 - 0.999 ** step) ** 0.5
    table = torch.from_numpy(tab.view(np.uint8)).to(dev)
    if guard is not None:
        table = guard.wrap(table, "segment table")
    out2 = ops.grad_norm(table, T, n_chunks, MAX_NORM)
    ops.adam_step(table, T, n_chunks, out2[1:])
    return [out2] + t["p"] + t["m"] + t["v"], t["g"]


def _snap(out):
    return [o.detach().cpu().clone() for o in out]


def _same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.numpy().tobytes() == y.numpy().tobytes(), "%s: output %d differs" % (what, i)


def test_three_fills_and_the_unguarded_run_are_bit_identical(dev, g):
    from gnnrag_amd import ops
    data, other = _data(1), _data(2)
    runs = []
    for fill, d in ((FILL_ZERO, data), (FILL_ZERO, other), (FILL_LEFTOVERS, data), (FILL_ONES, data)):
        g.fill = fill
        hits = g.leftover_hits
        out, _ = _run(g, dev, d)
        out = _snap(out)
        if fill == FILL_LEFTOVERS:
            assert g.leftover_hits >= hits + 2                      # out2 and the workspace ran in leftovers
        g.check("body fill %r" % (fill,))                           # guards, g and the table hold their bytes
        if d is data:
            runs.append(out)
    assert {"grad_norm: out2", "grad_norm: workspace"} <= set(g.sizes)
    assert g.sizes["grad_norm: workspace"] == ops._lib.load().gnnrag_optim_workspace_bytes(ops.optim_chunks(SIZES)[1])
    saved, ops._buf = ops._buf, g.plain
    try:
        plain = _snap(_run(None, dev, data)[0])
    finally:
        ops._buf = saved
    for what, r in (("leftovers", runs[1]), ("0xFF", runs[2]), ("unguarded", plain)):
        _same(runs[0], r, "0x00 run and %s run" % what)
    # the values: against the float64 formulas, the project's kernel tolerance
    total = np.sqrt(sum((x.astype(np.float64) ** 2).sum() for x in data["g"]))
    coef = min(1.0, MAX_NORM / (total + 1e-6))
    out2 = runs[0][0].numpy()
    assert abs(out2[0] - total) <= 2e-5 * total and abs(out2[1] - coef) <= 2e-5 * coef
    T, step = len(SIZES), 3
    for i in range(T):
        p, gr, m, v = (data[k][i].astype(np.float64) for k in "pgmv")
        gp = gr * coef + (0.01 if i % 2 else 0.0) * p
        m2 = m + (gp - m) * (1 - 0.9)
        v2 = v * 0.999 + (1 - 0.999) * gp * gp
        p2 = p - 1e-3 / (1 - 0.9 ** step) * m2 / (np.sqrt(v2) / (1 - 0.999 ** step) ** 0.5 + 1e-8)
        for got, want in ((runs[0][1 + i], p2), (runs[0][1 + T + i], m2), (runs[0][1 + 2 * T + i], v2)):
            assert np.abs(got.numpy() - want).max() <= 2e-5 * np.abs(want).max(), i


def test_one_byte_less_than_the_stated_workspace_is_refused(dev, g):
    from gnnrag_amd import _lib
    data = _data(3)
    _run(g, dev, data)
    g.check("the stated size")
    assert g.sizes["grad_norm: workspace"] > 16                     # above the binding's floor: the exact stated size
    g.short = {"grad_norm: workspace": 1}
    with pytest.raises(_lib.GnnragError) as e:
        _run(g, dev, data)
    g.short = {}
    m = re.search(r"failed \((-?\d+)\)", str(e.value))
    assert m and int(m.group(1)) == E_WORKSPACE
    g.check("one byte short")


def test_a_side_stream_call_gives_the_same_bits(dev, g):
    data = _data(4)
    scaled = dict(data, g=[x * 2 for x in data["g"]])

    def halve(gs):                                                  # the torch op right before the calls, on this stream
        return [x * 0.5 for x in gs]

    want = _snap(_run(g, dev, scaled, produce_g=halve)[0])
    g.check("default stream")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got, _ = _run(g, dev, scaled, produce_g=halve)
    side.synchronize()
    g.check("side stream")
    _same(want, _snap(got), "side stream")
    _same(want, _snap(_run(g, dev, data)[0]), "g from a torch op and g as given")
