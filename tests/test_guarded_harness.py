"""The guarded allocator of the tests (tests/guarded.py) proved on CPU tensors: it reports a write one element before and
one element after a view with the block's name and the offset, stays silent for in-bounds writes, and hands out
contiguous, exact-sized, 512-byte aligned views with the requested body fill."""
import numpy as np
import pytest
import torch

import guarded


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.uint8, torch.int16])
@pytest.mark.parametrize("shape", [(3, 5), 7, (2, 0, 4), (1,), (33, 30)])
def test_view_is_exact_contiguous_and_aligned(dtype, shape):
    g = guarded.Guard("cpu")
    t = g.alloc(shape, dtype, role="x")
    want = (shape,) if isinstance(shape, int) else tuple(shape)
    item = torch.empty(0, dtype=dtype).element_size()
    blk = g.blocks[-1]
    assert tuple(t.shape) == want and t.dtype == dtype and t.is_contiguous()
    assert t.numel() * item == blk.nbytes == int(np.prod(want)) * item
    assert guarded.GUARD_BYTES >= 64 * 1024 and guarded.GUARD_BYTES % 512 == 0
    assert blk.raw.numel() == 2 * guarded.GUARD_BYTES + blk.nbytes          # back guard starts right after the view
    assert t.storage_offset() * item == guarded.GUARD_BYTES                  # 512-byte aligned relative to its block
    if t.numel():                                                            # (an empty tensor has no address)
        assert (t.data_ptr() - blk.raw.data_ptr()) == guarded.GUARD_BYTES and guarded.GUARD_BYTES % 512 == 0
    g.check()


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
def test_body_fills(dtype):
    g = guarded.Guard("cpu")
    z = g.alloc((4, 3), dtype, fill=guarded.FILL_ZERO)
    assert (z == 0).all()
    f = g.alloc((4, 3), dtype, fill=guarded.FILL_ONES)
    assert torch.isnan(f).all() if dtype.is_floating_point else (f == -1).all()
    # the binding's own initialisation (zeros / NaN) survives whatever the body fill is
    g.fill = guarded.FILL_ONES
    assert (g.buf((2, 2), dtype, "cpu", "caller-zeroed", 0) == 0).all()
    if dtype.is_floating_point:
        assert torch.isnan(g.buf((2, 2), dtype, "cpu", "caller-nan", float("nan"))).all()
    assert (g.buf(5, dtype, "cpu", "left alone").view(torch.uint8) == 0xFF).all()
    g.check()


def test_leftovers_are_the_previous_buffer_of_the_role():
    g = guarded.Guard("cpu")
    a = g.alloc(6, torch.float32, role="op: out")
    a.copy_(torch.arange(6.0))
    g.alloc(6, torch.float32, role="op: other").fill_(9.0)
    g.fill = guarded.FILL_LEFTOVERS
    b = g.alloc(6, torch.float32, role="op: out")
    assert torch.equal(b, torch.arange(6.0)) and b.data_ptr() != a.data_ptr() and g.leftover_hits == 1
    c = g.alloc(8, torch.float32, role="op: out")           # no earlier buffer of this size: NaN bytes
    assert torch.isnan(c).all() and g.leftover_hits == 1
    g.check()


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
def test_out_of_bounds_writes_are_reported_with_block_and_offset(dtype):
    item = 4
    g = guarded.Guard("cpu")
    g.alloc((5, 3), dtype, role="op: first")
    t = g.alloc((5, 3), dtype, role="op: victim")
    g.alloc((5, 3), dtype, role="op: last")
    blk = g.blocks[1]
    whole = blk.raw.view(dtype)                              # the block as elements of the view's type
    first = guarded.GUARD_BYTES // item
    t.fill_(3)                                               # in bounds: silent
    t[4, 2] = 7
    t[0, 0] = 7
    g.check()
    assert whole[first] == 7 and whole[first + 14] == 7
    whole[first + 15] = 5                                    # one element after the view
    with pytest.raises(guarded.GuardError) as e:
        g.check("the call")
    msg = str(e.value)
    assert "op: victim, back guard, first bad byte +0" in msg and "op: first" not in msg and "op: last" not in msg
    assert msg.startswith("the call: ")
    whole[first + 15] = whole[first + 16]                    # repair, then one element before the view
    g.check()
    whole[first - 1] = 5
    with pytest.raises(guarded.GuardError) as e:
        g.check()
    assert "op: victim, front guard, first bad byte -4" in str(e.value)
    whole[first - 1] = whole[first - 2]
    blk.raw[guarded.GUARD_BYTES + blk.nbytes + 12] = 0x77    # a single byte further out
    with pytest.raises(guarded.GuardError) as e:
        g.check()
    assert "op: victim, back guard, first bad byte +12" in str(e.value)


def test_wrapped_inputs_keep_value_guards_and_are_watched():
    g = guarded.Guard("cpu")
    x = torch.randn(7, 3)
    idx = torch.arange(10, dtype=torch.int32)
    wx, wi = g.wrap(x, "op: x"), g.wrap(idx, "op: idx")
    assert torch.equal(wx, x) and torch.equal(wi, idx) and wx.data_ptr() != x.data_ptr()
    G = guarded.GUARD_BYTES
    assert (g.blocks[0].raw[:G] == 0xFF).all() and (g.blocks[0].raw[G + 84:] == 0xFF).all()     # NaN around floats
    assert (g.blocks[1].raw[:G] == 0).all() and (g.blocks[1].raw[G + 40:] == 0).all()           # index 0 around ints
    g.check()
    wx[2, 1] += 1.0                                          # a callee that scribbles on its input
    with pytest.raises(guarded.GuardError) as e:
        g.check()
    assert "op: x, input changed by the call, first changed byte 28" in str(e.value)


def test_install_replaces_the_bindings_allocator(monkeypatch):
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import ops
    plain = ops._buf((2, 3), torch.float32, "cpu", "role")
    assert tuple(plain.shape) == (2, 3) and plain.dtype == torch.float32
    assert (ops._buf(4, torch.int32, "cpu", "role", 0) == 0).all()
    assert torch.isnan(ops._buf((1, 2), torch.float32, "cpu", "role", float("nan"))).all()
    g = guarded.install(monkeypatch, guarded.Guard("cpu", fill=guarded.FILL_ONES))
    t = ops._buf((2, 3), torch.float32, "cpu", "linear: out")
    assert torch.isnan(t).all() and g.blocks[-1].role == "linear: out"


@pytest.mark.parametrize("F", [1, 7, 1000, 100003])
def test_narrow_tuple_stays_inside_its_host_block(F):
    """gnnrag_narrow_tuple (host code, no GPU): the [3, F] int32 block it fills sits between guards; the values are the
    narrowed ids whatever the block held, the int64 inputs are untouched, an id beyond int32 is refused (-4)."""
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(F)
    src = [torch.from_numpy(rng.integers(0, 2 ** 31, F)) for _ in range(3)]
    g = guarded.Guard("cpu")
    for fill in (guarded.FILL_ZERO, guarded.FILL_ONES):
        ins = [g.wrap(a, "narrow_tuple: ids %d" % i) for i, a in enumerate(src)]
        out = g.alloc((3, F), torch.int32, fill=fill, role="narrow_tuple: out")
        for threads in (1, 8):
            assert lib.gnnrag_narrow_tuple(ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), F, out.data_ptr(), threads) == 0
            g.check("narrow_tuple, %d threads" % threads)
            assert all(torch.equal(out[i].long(), src[i]) for i in range(3))
    bad = src[1].clone()
    bad[F // 2] = 2 ** 31
    assert lib.gnnrag_narrow_tuple(src[0].data_ptr(), bad.data_ptr(), src[2].data_ptr(), F, out.data_ptr(), 4) == _lib.E_TUPLE
    g.check("narrow_tuple, refused")
