"""Guarded-buffer tests of the C ABI (include/gnnrag.h: "caller-owned device memory", exact sizes, outputs "fully written
(not accumulated into)", "no state that affects results").  The value tests cannot see a kernel that writes a few rows past
a buffer, reads a workspace before it wrote it, or runs on another stream than the caller's; these can:

* every buffer the binding hands to the library (outputs, workspaces, structure memory, scratch: ``ops._buf``) and every
  input of the test is an exact-sized view between two 64 KiB guards (tests/guarded.py); after each call the guards and
  the inputs must hold their bytes;
* every call runs three times - buffers pre-filled with 0x00, then with the leftovers of a call on other inputs, then
  with 0xFF (NaN / -1) - in that order; where the suite already asserts bit-reproducibility the three results and the
  unguarded one are bit-identical, the forms with LDS float atomics stay within their existing tolerance; the 0x00 run
  is compared with the float64 oracle of the entry point's own value test, with that test's tolerance;
* stated sizes: ``gnnrag_*_bytes`` is enough (guards intact) and one byte less is refused with GNNRAG_E_WORKSPACE while
  the memory itself stays whole;
* side streams: an input produced on the side stream by a torch op right before the call, no wait in between.

No test here makes a kernel go out of bounds; the harness is shown to bite with a torch write (first test, and on CPU in
tests/test_guarded_harness.py).

Exported compute entry -> the test that guards it:
  gnnrag_csr_build, gnnrag_csr_build_counts, gnnrag_csr_status, gnnrag_csr_concat, gnnrag_csr_permute_weight,
  gnnrag_ugraph_build ............................ test_structure_builds
  gnnrag_narrow_tuple (host) ...................... test_guarded_harness.test_narrow_tuple_stays_inside_its_host_block
  gnnrag_relorder_build, gnnrag_aggregate_backward, gnnrag_aggregate_fused_backward, gnnrag_typelayer_backward
  ................................................ test_backward_kernels, test_empty_batch
  gnnrag_linear, gnnrag_linear_pair ............... test_linear_and_linear_pair
  gnnrag_rel_transform ............................ test_rel_transform_with_planes
  gnnrag_relation_tables, gnnrag_aggregate, gnnrag_aggregate_fused, gnnrag_typelayer
  ................................................ test_forward_kernels_of_a_layer, test_empty_batch
  gnnrag_aggregate_fused (each kernel), gnnrag_aggregate_fused_hub_form ... test_fused_walk_every_variant_and_hub_form
  gnnrag_relation_tables_planes ................... test_relation_tables_w_resident_and_planes
  gnnrag_update_score, gnnrag_update_score_fused .. test_update_score_both_forms
  gnnrag_masked_softmax ........................... test_masked_softmax
  gnnrag_gemm_tn .................................. test_gemm_tn
  gnnrag_frontier_build, gnnrag_relation_tables_frontier, gnnrag_aggregate_fused_frontier ... test_frontier_trio
  gnnrag_reason_layer ............................. test_reason_layer, test_layer_workspace_kept_across_shapes
  gnnrag_reason_stack, gnnrag_reason_stack_capture, gnnrag_graph_launch ... test_layer_stack_run_capture_replay, and the
  module forwards: test_random_sweep_cases_guarded, test_large_ragged_shape_guarded, test_c2_forward_guarded
  gnnrag_topp_candidates, gnnrag_topp_candidates_ws ... test_topp_candidates
  gnnrag_seed_retrieve, gnnrag_query_reform ....... test_seed_retrieve_and_query_reform
  gnnrag_lstm_forward ............................. test_lstm_forward
  gnnrag_shortest_paths ........................... test_selection_and_shortest_paths
  every byte count of the above ................... test_stated_sizes_are_sufficient_and_enforced
  side streams .................................... test_side_stream_calls_are_bit_identical
Left out: gnnrag_frontier_supported (a host predicate on the structure's fields: no buffer, no launch)."""
import dataclasses
import re

import numpy as np
import pytest
import torch

import guarded
from guarded import FILL_LEFTOVERS, FILL_ONES, FILL_ZERO

pytestmark = pytest.mark.gpu
TOL_KERNEL = 2e-5          # test_gpu_backward.py / test_gpu_parity.py TOL_INTERNAL: vs the float64 oracle
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
    ops._path_buffers.clear()                   # cached (unguarded) path buffers of earlier tests
    yield guard
    ops._path_buffers.clear()
    guard.release()


# -- helpers -----------------------------------------------------------------------------------------------------------

def _t(dev, *arrs):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]


def _f32(dev, *arrs):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in arrs]


def _snap(out):
    out = out if isinstance(out, (tuple, list)) else (out,)
    return [o.detach().cpu().clone() for o in out]


def _bits(t):
    return t.numpy().tobytes()


def _three(g, call, inputs, other, prepare=None):
    """``call(*tensors)`` in guarded buffers filled with 0x00, then (after a call on ``other`` inputs) with that call's
    leftovers, then with 0xFF; inputs wrapped, guards and inputs checked after every call.  ``prepare()`` drops what the
    binding caches between calls (workspaces of a plan), so that every fill reaches it.  Returns the three results."""
    runs = []
    for fill, inp in ((FILL_ZERO, inputs), (FILL_ZERO, other), (FILL_LEFTOVERS, inputs), (FILL_ONES, inputs)):
        g.fill = fill
        if prepare is not None:
            prepare()
        w = [None if t is None else g.wrap(t, "input %d" % i) for i, t in enumerate(inp)]
        hits, asked = g.leftover_hits, len(g.sizes)
        out = _snap(call(*w))
        if fill == FILL_LEFTOVERS and asked:            # the call allocated through the binding: it ran in leftovers
            assert g.leftover_hits > hits
        g.check("body fill %r%s" % (fill, "" if inp is inputs else " (other inputs)"))
        if inp is inputs:
            runs.append(out)
    return runs


def _plain(g, fn):
    """The same call the way every other test makes it: the binding's own allocator, unwrapped inputs."""
    from gnnrag_amd import ops
    saved, ops._buf = ops._buf, g.plain
    try:
        return _snap(fn())
    finally:
        ops._buf = saved


def _bit_identical(runs, plain=None, what=""):
    names = ["leftovers", "0xFF", "unguarded"]
    for k, r in enumerate(runs[1:] + ([plain] if plain is not None else [])):
        assert len(r) == len(runs[0])
        for i, (a, b) in enumerate(zip(runs[0], r)):
            assert a.shape == b.shape and a.dtype == b.dtype and _bits(a) == _bits(b), \
                "%s output %d: 0x00 run and %s run differ" % (what, i, names[k])


def _close(got, want, tol, msg, floor=1e-6):
    got = got.numpy() if isinstance(got, torch.Tensor) else got
    np.testing.assert_allclose(got, want, rtol=0, atol=tol * max(np.abs(want).max(), floor), err_msg=msg)


def _drop_workspaces(plan, relorder=False):
    """Forget the workspaces a plan caches (and, on demand, the backward's ordering): the next call allocates them again,
    with the body fill of the moment."""
    for key in [k for k in plan._w if isinstance(k, tuple) and (k[0] in ("ws", "bws") or (relorder and k[0] == "relorder"))]:
        del plan._w[key]


CASES = {   # test_gpu_backward.py CASES / test_gpu_parity.py: shapes whose kernel selection and oracles are known
    "hub": dict(B=3, N=600, E=4000, R=20, D=200, I=2, L=1, seed=3),
    "huge": dict(B=2, N=500, E=14000, R=20, D=200, I=2, L=1, seed=4),
    "odd": dict(B=2, N=33, E=150, R=5, D=30, I=3, L=1, seed=5, normalized_gnn=True),
    "wide": dict(B=2, N=40, E=160, R=4, D=300, I=1, L=1, seed=6),
    # the end of the buffer: B * N one more / one less than a multiple of 16 at D = 200, and B * N * D * 4 not a multiple
    # of 512 (17 * 47 * 200 * 4 = 639200 = 1248 * 512 + 224)
    "bn_plus1": dict(B=3, N=187, E=700, R=30, D=200, I=2, L=2, seed=11),        # 561 = 35 * 16 + 1
    "bn_minus1": dict(B=5, N=115, E=500, R=30, D=200, I=2, L=2, seed=12),       # 575 = 36 * 16 - 1
    "not512": dict(B=17, N=47, E=200, R=12, D=200, I=1, L=2, seed=13),          # 799 rows
}


def _cfg(name):
    from gnnrag_amd import synth
    return synth.CONFIGS[name] if name in synth.CONFIGS else synth.GraphConfig(name=name, **CASES[name])


def _plan(batch, dev, weights=True):
    from gnnrag_amd import ops
    cfg, et = batch.cfg, batch.edge_tuple
    plan = ops.CsrPlan(et[0], et[1], et[2], cfg.B, cfg.N, cfg.R1, dev)
    if weights and cfg.normalized_gnn:
        plan.attach_w_gnn(et[5])
    return plan


# -- the harness bites on the device -----------------------------------------------------------------------------------

def test_a_torch_write_past_a_guarded_device_view_is_reported(dev):
    g = guarded.Guard(dev)
    t = g.alloc((7, 50), torch.float32, role="probe: out")
    blk = g.blocks[-1]
    assert t.is_cuda and t.numel() * 4 == blk.nbytes == 1400 and t.data_ptr() % 512 == 0
    t.fill_(1.0)
    g.check()
    whole = blk.raw.view(torch.float32)
    whole[guarded.GUARD_BYTES // 4 + 350] = 2.0                  # one element after the view
    with pytest.raises(guarded.GuardError, match=r"probe: out, back guard, first bad byte \+0"):
        g.check()
    whole[guarded.GUARD_BYTES // 4 + 350] = float("nan")
    blk.raw[guarded.GUARD_BYTES + 1400: guarded.GUARD_BYTES + 1404] = 0xFF
    g.check()
    whole[guarded.GUARD_BYTES // 4 - 1] = 2.0                    # one element before it
    with pytest.raises(guarded.GuardError, match=r"probe: out, front guard, first bad byte -4"):
        g.check()


# -- structure builds --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["tiny", "tiny50", "tinyfb", "hub", "huge", "odd", "bn_plus1", "not512", "empty"])
def test_structure_builds(dev, g, name):
    """gnnrag_csr_build_counts (waiting and deferred form), gnnrag_csr_status, gnnrag_csr_concat,
    gnnrag_csr_permute_weight, gnnrag_relorder_build, gnnrag_ugraph_build: structure memory, scratch and the id block
    guarded; the arrays the structure exposes (``to_host``: only counted prefixes, gnnrag.h gnnrag_csr) are bit-identical
    whatever the memory held, equal to the unguarded build and to numpy (test_gpu_parity._csr_numpy,
    paths_oracle.ugraph_numpy)."""
    import paths_oracle
    from gnnrag_amd import ops, synth
    from test_gpu_parity import _csr_numpy
    if name == "empty":
        B, N, R1 = 2, 8, 3
        h = r = t = np.zeros(0, np.int64)
        wl = wrl = np.zeros(0, np.float32)
    else:
        cfg = _cfg(name)
        batch = synth.make_batch(cfg)
        B, N, R1 = cfg.B, cfg.N, cfg.R1
        h, r, t = (np.asarray(batch.edge_tuple[i]).astype(np.int64) for i in range(3))
        wl, wrl = (np.asarray(batch.edge_tuple[i], np.float32) for i in (5, 6))
    rng = np.random.default_rng(5)
    p = rng.permutation(len(h))                                   # "other inputs": the same facts in another order
    hrt = torch.from_numpy(np.stack([h, r, t]).astype(np.int32))
    pairs = np.unique(np.stack([h // N, r], 1), axis=0) if len(h) else np.zeros((0, 2), np.int64)
    per_q = np.bincount(pairs[:, 0], minlength=B) if len(pairs) else np.zeros(B, np.int64)
    counts = (int(per_q.sum()), int(per_q.max()))

    def build(form):
        def call(ids):
            if form == "wait":
                plan = ops.CsrPlan(None, None, None, B, N, R1, dev, hrt_device=ids) if ids.shape[1] else \
                    ops.CsrPlan(h, r, t, B, N, R1, dev)
            else:
                plan = ops.CsrPlan(None, None, None, B, N, R1, dev, hrt_device=ids, rel_counts=counts)
                plan.status()                                     # gnnrag_csr_status: the deferred validation
            plans.append(plan)
            if len(h):
                plan.attach_w_gnn(wl)
                plan.attach_w_rel(wrl)
            host = plan.to_host()
            out = [torch.from_numpy(np.ascontiguousarray(v)) for k, v in sorted(host.items()) if not isinstance(v, list)]
            out += [torch.from_numpy(np.ascontiguousarray(x)) for x in host["big"]]
            if len(h):
                ug = ops.UGraph(plan).to_host()
                out += [torch.from_numpy(ug["u_ptr"]), torch.from_numpy(np.ascontiguousarray(ug["u_adj"]))]
            return out
        return call

    for form in (["wait", "counts"] if len(h) else ["wait"]):
        plans = []
        other = [hrt[:, torch.from_numpy(p)].contiguous().to(dev)] if len(h) else [hrt.to(dev)]
        runs = _three(g, build(form), [hrt.to(dev)], other)
        plain = _plain(g, lambda: build(form)(hrt.to(dev)))
        _bit_identical(runs, plain, "%s build" % form)
    got = plans[0].to_host()
    want = _csr_numpy(h, r, t, B, N, R1)
    for k, v in want.items():
        np.testing.assert_array_equal(got[k], v, err_msg=k)
    np.testing.assert_array_equal(got["rel_rows"], pairs)
    assert (plans[0].rel_total, plans[0].rel_max) == counts
    if len(h) == 0:
        return
    for d in (0, 1):
        np.testing.assert_array_equal(got["w_gnn"][d], (wl * wl)[want["perm%d" % d]])
        np.testing.assert_array_equal(got["w_rel"][d], wrl[want["perm%d" % d]])
    u_ptr, u_adj = paths_oracle.ugraph_numpy(h, t, B * N)
    ug = ops.UGraph(plans[0]).to_host()
    assert np.array_equal(ug["u_ptr"], u_ptr) and np.array_equal(ug["u_adj"], u_adj)
    # gnnrag_csr_build itself (the binding always goes through gnnrag_csr_build_counts), weights inside the structure
    import ctypes as C
    from gnnrag_amd import _lib
    lib = _lib.load()
    F = len(h)
    for fill in (FILL_ZERO, FILL_ONES):
        g.fill = fill
        ids, w1, w2 = g.wrap(hrt.to(dev), "csr_build: ids"), g.wrap(torch.from_numpy(wl).to(dev), "csr_build: w_gnn"), \
            g.wrap(torch.from_numpy(wrl).to(dev), "csr_build: w_rel")
        own = ops.CsrPlan.__new__(ops.CsrPlan)
        own.B, own.N, own.R1, own.F, own.device, own._w = B, N, R1, F, dev, {}
        own._mem = ops._buf(lib.gnnrag_csr_bytes(F, B, N, R1, 1, 1), torch.uint8, dev, "csr_build: csr_mem (weights)")
        scratch = ops._buf(lib.gnnrag_csr_scratch_bytes(F, B, N, R1), torch.uint8, dev, "csr_build: scratch")
        own.c = _lib.CsrStruct()
        _lib.check(lib.gnnrag_csr_build(ids[0].data_ptr(), ids[1].data_ptr(), ids[2].data_ptr(), w1.data_ptr(), w2.data_ptr(),
                                        F, B, N, R1, own._mem.data_ptr(), own._mem.numel(), scratch.data_ptr(),
                                        scratch.numel(), C.byref(own.c), torch.cuda.current_stream().cuda_stream),
                   "gnnrag_csr_build")
        own.rel_total, own.rel_max = int(own.c.rel_total), int(own.c.rel_max)
        g.check("gnnrag_csr_build, body fill %r" % (fill,))
        mine = own.to_host()
        for k, v in got.items():
            if k in ("w_gnn", "w_rel"):
                for d in (0, 1):        # the same sorted weights the lazy attach gave above (w_gnn squared, w_rel as is)
                    stored = own._view(getattr(own.c, k)[d], F, torch.float32).numpy()
                    assert np.array_equal(stored, v[d]), k
            elif isinstance(v, list):
                assert all(np.array_equal(x, y) for x, y in zip(v, mine[k])), k
            else:
                assert np.array_equal(v, mine[k]), k
    # the batch as a concatenation of per-question structures: bit-identical to the build from the batch tuple
    q = h // N

    def concat(ids):
        parts = []
        for b in range(B):
            m = torch.from_numpy(q == b)
            sub = ids[:, m.to(ids.device)].clone()
            sub[0] -= b * N
            sub[2] -= b * N
            parts.append(ops.CsrPlan(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), 1, N, R1, dev)
                         if sub.shape[1] == 0 else ops.CsrPlan(None, None, None, 1, N, R1, dev, hrt_device=sub.contiguous()))
        whole = ops.CsrPlan.concat(parts, N, R1, dev)
        host = whole.to_host()
        return [torch.from_numpy(np.ascontiguousarray(host[k])) for k in
                ("row_ptr0", "row_ptr1", "edge0", "edge1", "perm0", "perm1", "rel_off", "rel_rows", "edge_m", "m_dst")]

    runs = _three(g, concat, [hrt.to(dev)], [hrt.to(dev)])
    _bit_identical(runs, None, "concat")
    for k, v in zip(("row_ptr0", "row_ptr1", "edge0", "edge1", "perm0", "perm1", "rel_off", "rel_rows", "edge_m", "m_dst"),
                    runs[0]):
        if not k.startswith("perm"):            # fact ids: the parts number their own facts
            np.testing.assert_array_equal(v.numpy(), got[k], err_msg="concat " + k)


# -- dense kernels -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("math", [0, 1, 2], ids=["fp32", "bf16x3", "mixed"])
@pytest.mark.parametrize("M,K,Nout,with_add,relu", [(602, 200, 200, True, False), (9, 50, 50, True, True),
                                                    (257, 1000, 200, False, True), (4099, 250, 50, False, True),
                                                    (33, 30, 30, False, False), (8209, 200, 200, False, True),
                                                    (16391, 200, 200, True, True), (16391, 36, 216, True, True),
                                                    (16391, 30, 72, False, False)])
def test_linear_and_linear_pair(dev, g, math, M, K, Nout, with_add, relu):
    """gnnrag_linear and gnnrag_linear_pair in every math mode against fp64, tolerance of test_linear_vs_fp64; M not a
    multiple of the row tile.  Up to 16384 rows both run k_gemm_skinny (the pair in one launch); the 16391-row shapes
    run k_gemm_f32 - the pair as two gnnrag_linear calls - with `add` and relu, a second column block (Nout = 216) and
    the scalar loaders (K = 30).  There is no W-resident kernel for these entry points."""
    from gnnrag_amd import _lib, ops
    lib = _lib.load()
    for entry in ("linear", "linear_pair"):
        f = ops.dense_form(entry, M, K, Nout, math=math, add_rows=max(M - 1, 1) if with_add else None)
        if M <= 16384:
            assert (f.family, f.launches) == (ops.DENSE_SKINNY, 1)
        else:
            assert f.family == ops.DENSE_KTILED and f.math == int(math != 0 and K % 4 == 0)
            assert f.launches == (Nout + 207) // 208 * (2 if entry == "linear_pair" else 1)

    def data(seed):
        rng = np.random.default_rng(seed)
        A = [rng.standard_normal((M, K)).astype(np.float32) for _ in range(2)]
        W = (rng.standard_normal((Nout, K)) / np.sqrt(K)).astype(np.float32)
        b = rng.standard_normal(Nout).astype(np.float32)
        add = [rng.standard_normal((max(M - 1, 1), Nout)).astype(np.float32) if with_add else None for _ in range(2)]
        return [A[0], A[1], W, b, add[0], add[1]]

    def want(A0, A1, W, b, add0, add1, d, act):
        w = (A0, A1)[d].astype(np.float64) @ W.astype(np.float64).T + b
        if add0 is not None:
            w[: add0.shape[0]] += (add0, add1)[d]
        return np.maximum(w, 0) if act else w

    def call(A0, A1, W, b, add0, add1):
        one = ops.linear(A0, W, b, add0, relu=relu, math=math)
        C0 = ops._buf((M, Nout), torch.float32, dev, "linear_pair: C0")
        C1 = ops._buf((M, Nout), torch.float32, dev, "linear_pair: C1")
        _lib.check(lib.gnnrag_linear_pair(A0.data_ptr(), A1.data_ptr(), M, K, W.data_ptr(), b.data_ptr(),
                                          None if add0 is None else add0.data_ptr(),
                                          None if add1 is None else add1.data_ptr(),
                                          0 if add0 is None else add0.shape[0], C0.data_ptr(), C1.data_ptr(), Nout, math,
                                          torch.cuda.current_stream().cuda_stream), "gnnrag_linear_pair")
        return one, C0, C1

    d0, d1 = data(M + K), data(M + K + 1)
    runs = _three(g, call, _t(dev, *d0), _t(dev, *d1))
    tol = 5e-6 * np.sqrt(K)
    for run in runs:
        np.testing.assert_allclose(run[0].numpy(), want(*d0, 0, relu), rtol=0, atol=tol)
        np.testing.assert_allclose(run[1].numpy(), want(*d0, 0, False), rtol=0, atol=tol)      # the pair has no relu
        np.testing.assert_allclose(run[2].numpy(), want(*d0, 1, False), rtol=0, atol=tol)
    _bit_identical(runs, _plain(g, lambda: call(*_t(dev, *d0))), "linear")


@pytest.mark.parametrize("R1,D,L,pos_rows", [(602, 200, 3, 602), (12, 56, 2, 7), (1, 8, 1, 0), (130, 36, 9, 130),
                                             (3001, 208, 2, 2500)])
def test_rel_transform_with_planes(dev, g, R1, D, L, pos_rows):
    """gnnrag_rel_transform: all layers' projections and (D <= 224) the bf16 planes of relu(+-T): against fp64 with
    test_rel_transform_all_layers_in_one_launch_vs_fp64's tolerance; planes sum EXACTLY to relu(+-T) and their padding
    is zero (test_relation_tables_from_relation_planes) under every fill."""
    from gnnrag_amd import ops

    def data(seed):
        rng = np.random.default_rng(seed)
        arrs = [rng.standard_normal((R1, D)).astype(np.float32) for _ in range(2)]
        for j in range(L):
            arrs += [(rng.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32), rng.standard_normal(D).astype(np.float32)]
            arrs += [rng.standard_normal((pos_rows, D)).astype(np.float32) for _ in range(2)] if pos_rows else [None, None]
        return arrs

    def call(A0, A1, *rest):
        layers = [tuple(rest[4 * j: 4 * j + 4]) for j in range(L)]
        return ops.rel_transform(A0, A1, layers, planes=True)

    d0, d1 = data(R1 + D + L), data(R1 + D + L + 1)
    runs = _three(g, call, _t(dev, *d0), _t(dev, *d1))
    want = np.zeros((L, 2, R1, D))
    for j in range(L):
        W, b, pos = d0[2 + 4 * j], d0[3 + 4 * j], d0[4 + 4 * j: 6 + 4 * j]
        for d in range(2):
            want[j, d] = d0[d].astype(np.float64) @ W.astype(np.float64).T + b
            if pos_rows:
                want[j, d, :pos_rows] += pos[d]
    for T, planes in runs:
        np.testing.assert_allclose(T.numpy(), want, rtol=0, atol=5e-6 * np.sqrt(D))
        Tn = T.numpy()
        as_f32 = (planes.numpy().view(np.uint16).astype(np.uint32) << 16).view(np.float32)
        total = as_f32[:, :, 0].astype(np.float64) + as_f32[:, :, 1] + as_f32[:, :, 2]
        assert np.array_equal(total[..., :D], np.maximum(Tn, 0).astype(np.float64))
        assert np.array_equal(total[..., 224:224 + D], np.maximum(-Tn, 0).astype(np.float64))
        pl = planes.numpy()
        assert not pl[..., D:224].any() and not pl[..., 224 + D:].any()
    _bit_identical(runs, _plain(g, lambda: call(*_t(dev, *d0))), "rel_transform")


@pytest.mark.parametrize("M,N1,N2", [(1000, 200, 200), (4097, 200, 1000), (37, 8, 12), (1, 4, 4), (5000, 56, 56),
                                     (70000, 200, 400)])
def test_gemm_tn(dev, g, M, N1, N2):
    """gnnrag_gemm_tn (C accumulated over row chunks after an internal memset): bit-identical under every fill
    (test_gemm_tn_weight_gradient_vs_fp64 asserts the fixed order), fp64 within its 1e-5."""
    from gnnrag_amd import ops
    rng = np.random.default_rng(M + N1)
    d0 = [rng.standard_normal((M, N1)).astype(np.float32), rng.standard_normal((M, N2)).astype(np.float32)]
    d1 = [rng.standard_normal((M, N1)).astype(np.float32), rng.standard_normal((M, N2)).astype(np.float32)]
    runs = _three(g, ops.gemm_tn, _t(dev, *d0), _t(dev, *d1))
    _close(runs[0][0], d0[0].astype(np.float64).T @ d0[1].astype(np.float64), 1e-5, "gemm_tn")
    _bit_identical(runs, _plain(g, lambda: ops.gemm_tn(*_t(dev, *d0))), "gemm_tn")


@pytest.mark.parametrize("math", [0, 1], ids=["fp32", "bf16x3"])
@pytest.mark.parametrize("M,D,I", [(8192, 200, 2), (9008, 200, 2), (8192, 208, 2), (9008, 208, 2), (16001, 200, 2),
                                   (15999, 200, 1), (799, 200, 1), (66, 30, 3), (80, 300, 1), (9001, 56, 2)])
def test_update_score_both_forms(dev, g, math, M, D, I):
    """gnnrag_update_score and gnnrag_update_score_fused (W-resident bf16x3 / fp32 kernels and the k-tiled one; ragged
    last 16-row tile; the score is accumulated across column blocks after an internal memset): fp64 within the
    tolerances of test_aggregate_and_update_vs_np64 / test_update_bf16x3_w_resident_vs_exact_fp32 under every fill;
    masked slots exactly -1e11."""
    from gnnrag_amd import ops

    def data(seed):
        gen = torch.Generator(device="cpu").manual_seed(seed)
        r = lambda *shape: torch.randn(*shape, generator=gen)
        return [r(M, D), r(M, D), r(M, 2 * I * D) / 4, r(D, (2 * I + 1) * D) / 14, r(D), r(D), r(1),
                (torch.rand(M, generator=gen) > 0.1).float()]

    def call(h, nbr, agg, W, b, ws, bs, mask):
        return ops.update_score_fused(h, nbr, W, b, ws, bs, mask, I, math=math) + \
            ops.update_score(h, agg, W, b, ws, bs, mask, I, math=math)

    d0, d1 = data(M + D), data(M + D + 1)
    runs = _three(g, call, [x.to(dev) for x in d0], [x.to(dev) for x in d1])
    h, nbr, agg, W, b, ws, bs, mask = (x.double().numpy() for x in d0)
    live = mask > 0
    wants = []
    for pre in (h @ W[:, :D].T + nbr + b, np.concatenate([h, agg], 1) @ W.T + b):
        hn = np.maximum(pre, 0)
        wants.append((hn, hn @ ws + bs))
    for run in runs:
        for k, (hn, sc) in enumerate(wants):
            got_h, got_s = run[2 * k].numpy(), run[2 * k + 1].numpy()
            assert np.abs(got_h - hn).max() <= TOL_KERNEL * max(1.0, np.abs(hn).max()), (k, np.abs(got_h - hn).max())
            assert np.abs(got_s - sc)[live].max() <= 1e-4 * max(1.0, np.abs(sc[live]).max())
            assert (got_s[~live] == np.float32(-1e11)).all()


@pytest.mark.parametrize("B,N", [(3, 48), (5, 2047), (2, 3000), (7, 33), (1, 1)])
def test_masked_softmax(dev, g, B, N):
    from gnnrag_amd import ops

    def data(seed):
        rng = np.random.default_rng(seed)
        s = rng.standard_normal((B, N)).astype(np.float32) * 3
        s[rng.random((B, N)) < 0.3] = -1e11
        if B > 2:
            s[2] = -1e11                                            # an all-masked question: uniform, like the reference
        return [s]

    d0, d1 = data(B + N), data(B * N + 1)
    runs = _three(g, lambda s: ops.masked_softmax(s, B, N), _t(dev, *d0), _t(dev, *d1))
    s = d0[0].astype(np.float64)
    e = np.exp(s - s.max(1, keepdims=True))
    for run in runs:
        np.testing.assert_allclose(run[0].numpy(), e / e.sum(1, keepdims=True), rtol=0, atol=1e-6)
    _bit_identical(runs, _plain(g, lambda: ops.masked_softmax(*_t(dev, *d0), B, N)), "masked_softmax")


@pytest.mark.parametrize("B,N,D,ld", [(3, 70, 50, 50), (20, 500, 200, 200), (2, 130, 300, 300), (3, 70, 50, 64), (1, 2000, 50, 56)])
def test_seed_retrieve_and_query_reform(dev, g, B, N, D, ld):
    """gnnrag_seed_retrieve / gnnrag_query_reform (also on a zero-padded node state read in place, ld > D) against the
    float64 statement of query_update.py:26-44; tolerances of test_query_reform_seed_retrieve (1e-6 / 4e-6)."""
    from gnnrag_amd import ops

    def data(seed):
        gen = torch.Generator().manual_seed(seed)
        ent = torch.zeros(B, N, ld)
        ent[..., :D] = torch.randn(B, N, D, generator=gen)
        s = torch.zeros(B, N)
        s[:, 0] = 1.0
        if B > 1:
            s[1, N - 1] = 0.5
            s[1, 0] = 0.5
        if B > 2:
            s[2] = 0.0
        u = lambda: (torch.rand(D, 3 * D, generator=gen) * 2 - 1) / np.sqrt(3 * D)       # nn.Linear's own init range
        return [torch.randn(B, D, generator=gen), s, ent, u(), u()]

    def call(q, s, ent, Wr, Wg):
        return ops.seed_retrieve(s, ent), ops.query_reform(q, s, ent, Wr, Wg)

    d0, d1 = data(B + N), data(B + N + 1)
    runs = _three(g, call, [x.to(dev) for x in d0], [x.to(dev) for x in d1])
    q, s, ent, Wr, Wg = (x.double() for x in d0)
    y = torch.bmm(s.unsqueeze(1), ent).squeeze(1)
    feats = torch.cat([q, y[:, :D], q - y[:, :D]], 1)
    gate = torch.sigmoid(feats @ Wg.T)
    want = gate * (feats @ Wr.T) + (1 - gate) * q
    for run in runs:
        assert (run[0].double() - y).abs().max().item() <= 1e-6
        assert (run[1].double() - want).abs().max().item() <= 4e-6
    _bit_identical(runs, _plain(g, lambda: call(*[x.to(dev) for x in d0])), "query_reform")


@pytest.mark.parametrize("B,T,E,H", [(16, 9, 300, 200), (1, 1, 300, 50), (3, 13, 300, 50), (20, 7, 64, 256), (513, 5, 100, 52)])
def test_lstm_forward(dev, g, B, T, E, H):
    """gnnrag_lstm_forward (out, h_n, c_n and the transposed-weight workspace guarded): the float64 oracle
    (oracle/lstm_np64.py) within test_gpu_lstm.py's 2e-5 (4x for c); one fixed summation order, so bit-identical."""
    import oracle.lstm_np64 as lstm_np64
    from gnnrag_amd import ops

    def data(seed):
        torch.manual_seed(seed)
        ref = torch.nn.LSTM(E, H, batch_first=True)
        return [torch.randn(B, T, E)] + [p.detach().clone() for p in (ref.weight_ih_l0, ref.weight_hh_l0, ref.bias_ih_l0,
                                                                       ref.bias_hh_l0)] + [0.3 * torch.randn(B, H), 0.3 * torch.randn(B, H)]

    def call(x, wi, wh, bi, bh, h0, c0):
        return ops.lstm_forward(x, wi, wh, bi, bh) + ops.lstm_forward(x, wi, wh, None, None, h0, c0)

    d0, d1 = data(B + T), data(B + T + 1)
    runs = _three(g, call, [x.to(dev) for x in d0], [x.to(dev) for x in d1])
    x, wi, wh, bi, bh, h0, c0 = (a.numpy() for a in d0)
    want = tuple(lstm_np64.lstm_forward(x, wi, wh, bi, bh))
    want += lstm_np64.lstm_forward(x, wi, wh, None, None, h0, c0)
    for k, w in enumerate(want):
        assert np.abs(runs[0][k].numpy() - w).max() <= (4 if k % 3 == 2 else 1) * 2e-5, k
    _bit_identical(runs, _plain(g, lambda: call(*[x.to(dev) for x in d0])), "lstm_forward")


@pytest.mark.parametrize("B,N", [(3, 48), (4, 2000), (2, 16384), (2, 20000), (3, 16391)])
def test_topp_candidates(dev, g, B, N):
    """gnnrag_topp_candidates_ws in the LDS form and (N > 16384) the workspace form: out_slot is specified in full
    ("the kept slots in that order, then -1", gnnrag.h), so all of it is compared; against numpy's stable sort."""
    from gnnrag_amd import _lib, ops

    def data(seed):
        rng = np.random.default_rng(seed)
        p = rng.dirichlet(np.ones(N) * 0.05, size=B).astype(np.float32)
        p[:, rng.integers(0, N, 5)] = p[:, :1]                    # ties
        el = (rng.random((B, N)) > 0.2).astype(np.uint8)
        if B > 2:
            el[2] = 0                                              # nothing eligible
        return [p, el]

    eps, ign = 0.95, 0.05 / N
    assert (_lib.load().gnnrag_topp_workspace_bytes(B, N) > 0) == (N > 16384)
    d0, d1 = data(B + N), data(B + N + 1)
    lib = _lib.load()

    def call(p, el):
        out = ops.topp_candidates(p, el, ign, eps)
        if N <= 16384:                                           # gnnrag_topp_candidates: the entry without a workspace
            slots = ops._buf((B, N), torch.int32, dev, "topp_candidates: slots")
            cnt = ops._buf((B, 2), torch.int32, dev, "topp_candidates: counts")
            _lib.check(lib.gnnrag_topp_candidates(p.data_ptr(), el.data_ptr(), B, N, ign, eps, slots.data_ptr(),
                                                  cnt.data_ptr(), torch.cuda.current_stream().cuda_stream), "gnnrag_topp_candidates")
            out += (slots, cnt)
        return out

    runs = _three(g, call, _t(dev, *d0), _t(dev, *d1))
    p, el = d0
    slots, cnt = np.full((B, N), -1, np.int32), np.zeros((B, 2), np.int32)
    for b in range(B):
        keep = np.flatnonzero((el[b] != 0) & (p[b].astype(np.float64) >= ign))
        order = keep[np.argsort(-p[b][keep], kind="stable")]
        slots[b, : len(order)] = order
        run = np.cumsum(p[b][order].astype(np.float64))
        over = np.flatnonzero(run > eps)
        cnt[b] = (len(order), over[0] + 1 if len(over) else len(order))
    for k in range(0, len(runs[0]), 2):
        assert np.array_equal(runs[0][k].numpy(), slots) and np.array_equal(runs[0][k + 1].numpy(), cnt)
    _bit_identical(runs, _plain(g, lambda: call(*_t(dev, *d0))), "topp")


# -- graph kernels -----------------------------------------------------------------------------------------------------

GRAPH_CASES = ["tiny", "tiny50", "tinyfb", "hub", "huge", "odd", "wide", "bn_plus1", "bn_minus1", "not512"]


def _layer_data(cfg, seed):
    """Inputs of the per-kernel calls of one layer: prior (sparse every third node), instructions, both relation
    projections, e2e weight, node state, cotangents."""
    rng = np.random.default_rng(seed)
    B, N, D, I = cfg.B, cfg.N, cfg.D, cfg.I
    dist = rng.random((B, N)).astype(np.float32)
    dist[:, ::3] = 0.0
    dist /= dist.sum(1, keepdims=True)
    return dict(dist=dist, ins=(0.5 * rng.standard_normal((B, I, D))).astype(np.float32),
                T_f=(0.5 * rng.standard_normal((cfg.R1, D))).astype(np.float32),
                T_i=(0.5 * rng.standard_normal((cfg.R1, D))).astype(np.float32),
                W=rng.uniform(-0.05, 0.05, size=(D, (2 * I + 1) * D)).astype(np.float32),
                g_agg=rng.standard_normal((B * N, 2 * I * D)).astype(np.float32),
                g_nbr=rng.standard_normal((B * N, D)).astype(np.float32))


def _tables_f64(plan, d, cfg):
    rows = plan.rel_rows()
    D, I = cfg.D, cfg.I
    want = np.zeros((2, plan.rel_total, D))
    for dd, Tt in enumerate((d["T_f"], d["T_i"])):
        for i in range(I):
            A = np.maximum(Tt[rows[:, 1]].astype(np.float64) * d["ins"][rows[:, 0], i].astype(np.float64), 0.0)
            want[dd] += A @ d["W"][:, (1 + 2 * i + dd) * D:(2 + 2 * i + dd) * D].astype(np.float64).T
    return want


def _walk_f64(plan, batch, dist, P):
    """nbr, and with a cotangent the gradients, as float64 sums over the caller's fact tuple
    (test_fused_walk_backward_vs_f64)."""
    cfg, et = batch.cfg, batch.edge_tuple
    h, r, t = (np.asarray(et[k]).astype(np.int64) for k in range(3))
    w = np.asarray(et[5], dtype=np.float64) ** 2 if cfg.normalized_gnn else np.ones(len(h))
    rows = plan.rel_rows().astype(np.int64)
    key = rows[:, 0] * (cfg.R1 + 1) + rows[:, 1]
    row_of = np.searchsorted(key, (h // cfg.N) * (cfg.R1 + 1) + r)
    d64, P64 = dist.reshape(-1).astype(np.float64), P.astype(np.float64)
    nbr = np.zeros((cfg.B * cfg.N, cfg.D))
    np.add.at(nbr, t, (w * d64[h])[:, None] * P64[0][row_of])
    np.add.at(nbr, h, (w * d64[t])[:, None] * P64[1][row_of])
    return nbr, (h, t, w, row_of, d64, P64)


@pytest.mark.parametrize("name", GRAPH_CASES)
def test_forward_kernels_of_a_layer(dev, g, name):
    """gnnrag_relation_tables (exact fp32 and bf16x3), gnnrag_aggregate, gnnrag_aggregate_fused, gnnrag_typelayer on one
    structure: tables / agg / nbr / h0 against float64 sums over the caller's fact tuple (2e-5 of the largest entry, as
    test_fused_kernels_vs_np64 / test_fused_walk_backward_vs_f64); the fused walk is bit-identical under every fill."""
    import oracle.rearev_grad as og
    from gnnrag_amd import ops, synth
    cfg = _cfg(name)
    batch = synth.make_batch(cfg)
    plan = _plan(batch, dev)
    plan.attach_w_rel(batch.edge_tuple[6])
    et = batch.edge_tuple
    d0, d1 = _layer_data(cfg, 17), _layer_data(cfg, 18)
    keys = ("dist", "ins", "T_f", "T_i", "W")

    def call(dist, ins, T_f, T_i, W):
        P32 = ops.relation_tables(plan, T_f, T_i, ins, W, math=ops.MATH_FP32)
        Pb3 = ops.relation_tables(plan, T_f, T_i, ins, W, math=ops.MATH_BF16X3)
        return (P32, Pb3, ops.aggregate(plan, dist, ins, T_f, T_i), ops.aggregate_fused(plan, dist, P32),
                ops.typelayer(plan, T_f, False), ops.typelayer(plan, T_f, True))

    runs = _three(g, call, _t(dev, *[d0[k] for k in keys]), _t(dev, *[d1[k] for k in keys]), lambda: _drop_workspaces(plan))
    want_P = _tables_f64(plan, d0, cfg)
    weight = et[5] if cfg.normalized_gnn else None
    want_agg = og.aggregate_grads(et, cfg.B, cfg.N, d0["dist"], d0["ins"], d0["T_f"], d0["T_i"], d0["g_agg"], weight)[0]
    for run in runs:
        _close(run[0], want_P, TOL_KERNEL, "P fp32", floor=1.0)
        _close(run[1], want_P, TOL_KERNEL, "P bf16x3", floor=1.0)
        _close(run[2], want_agg.reshape(cfg.B * cfg.N, -1), TOL_KERNEL, "agg")
        want_nbr, _ = _walk_f64(plan, batch, d0["dist"], run[0].numpy())
        _close(run[3], want_nbr, TOL_KERNEL, "nbr")
    # gnnrag.h: h0 = relu(sum over the facts at n, both sides, of v_f T[rel_f]) - oracle/rearev_grad.typelayer_pre
    for k, wr in ((4, None), (5, et[6])):
        want = np.maximum(og.typelayer_pre(et, cfg.B, cfg.N, torch.from_numpy(d0["T_f"]).double(), wr).numpy(), 0)
        for run in runs:
            _close(run[k], want.reshape(run[k].shape), TOL_KERNEL, "typelayer", floor=1.0)
    plain = _plain(g, lambda: call(*_t(dev, *[d0[k] for k in keys])))
    _bit_identical([[r[3]] for r in runs], [plain[3]], "aggregate_fused (%s)" % ops.WALK_KERNEL_NAMES[
        ops.aggregate_fused_variant(plan, cfg.D)].split(" ")[0])


@pytest.mark.parametrize("case", ["dense", "chunked", "weights", "lds16", "lds32"])
def test_fused_walk_every_variant_and_hub_form(dev, g, case):
    """gnnrag_aggregate_fused on each kernel it dispatches - the gather walk with the dense hub product, with the chunked
    fallback (weight blocks larger than their workspace region) and with per-fact weights (test_gpu_hub_rows.py graphs),
    the 16- and 32-column LDS walks - the kernel that ran asserted from gnnrag_aggregate_fused_variant /
    gnnrag_aggregate_fused_hub_form (whose 4-int output is guarded too); float64 within 2e-5, bit-identical."""
    from gnnrag_amd import ops, synth
    from test_gpu_hub_rows import _graph, _graph_blocks_do_not_fit
    D = 200
    if case in ("dense", "chunked", "weights"):
        B, N, R, h, r, t = (_graph_blocks_do_not_fit if case == "chunked" else _graph)()
        want_variant = ops.WALK_L2_GATHER
        want_form = ops.HUB_FORM_CHUNKED if case == "chunked" else ops.HUB_FORM_DENSE
    else:
        # the host picks the slice width from rel_max and D: the first candidate shape that lands on the wanted kernel
        want_variant = ops.WALK_LDS_16 if case == "lds16" else ops.WALK_LDS_32
        want_form = ops.HUB_FORM_NONE
        for cfg in (synth.GraphConfig(name=case, B=4, N=2000, E=10000, R=600, seed=5), _cfg("hub"), _cfg("tiny"),
                    synth.GraphConfig(name=case, B=3, N=900, E=4000, R=150, seed=6),
                    synth.GraphConfig(name=case, B=3, N=900, E=4000, R=300, seed=7)):
            batch = synth.make_batch(cfg)
            B, N, R = cfg.B, cfg.N, cfg.R1
            h, r, t = (np.asarray(batch.edge_tuple[k]).astype(np.int64) for k in range(3))
            if ops.aggregate_fused_variant(ops.CsrPlan(h, r, t, B, N, R, dev), D) == want_variant:
                break
    plan = ops.CsrPlan(h, r, t, B, N, R, dev)
    assert ops.aggregate_fused_variant(plan, D) == want_variant
    rng = np.random.default_rng(9)
    wfact = None
    if case == "weights":
        wfact = (0.5 + rng.random(len(h))).astype(np.float32)
        plan.attach_w_gnn(wfact)
    g.check("build")
    form = ops.aggregate_fused_hub_form(plan, D, 1)
    g.check("hub_form")
    import os
    if os.environ.get("GNNRAG_HUB_DENSE") != "0":
        assert form["form"] == want_form, form

    def data():
        dist = rng.random((B, N)).astype(np.float32)
        dist[:, ::3] = 0.0
        return [dist, (rng.standard_normal((2, plan.rel_total, D)) * 0.3).astype(np.float32)]

    d0, d1 = data(), data()
    runs = _three(g, lambda dist, P: ops.aggregate_fused(plan, dist, P), _t(dev, *d0), _t(dev, *d1),
                  lambda: _drop_workspaces(plan))
    rows = plan.rel_rows().astype(np.int64)
    key = rows[:, 0] * (R + 1) + rows[:, 1]
    row_of = np.searchsorted(key, (h // N) * (R + 1) + r)
    want = np.zeros((B * N, D))
    d64 = d0[0].reshape(-1).astype(np.float64)
    w2 = np.ones(len(h)) if wfact is None else wfact.astype(np.float64) ** 2
    np.add.at(want, t, (w2 * d64[h])[:, None] * d0[1][0][row_of].astype(np.float64))
    np.add.at(want, h, (w2 * d64[t])[:, None] * d0[1][1][row_of].astype(np.float64))
    assert np.abs(runs[0][0].numpy() - want).max() <= TOL_KERNEL * np.abs(want).max()
    _bit_identical(runs, _plain(g, lambda: ops.aggregate_fused(plan, *_t(dev, *d0))), case)


@pytest.mark.parametrize("B,R,used,I,N,D", [(9, 1500, 260, 3, 1500, 200), (5, 500, None, 2, 1000, 208)])
def test_relation_tables_w_resident_and_planes(dev, g, B, R, used, I, N, D):
    """The W-resident bf16x3 table kernel and the V form from relation planes (gnnrag_relation_tables_planes) at a row
    count that is not a multiple of 16 (test_relation_tables_bf16x3_w_resident_kernel's ragged case) and at D = 208."""
    from gnnrag_amd import ops, synth
    cfg = synth.GraphConfig(name="tab", B=B, N=N, E=6 * N, R=R, D=D, I=I, L=1, T=1, seed=B + R, rel_per_question=used,
                            n_real_min=N // 3)
    batch = synth.make_batch(cfg)
    plan = _plan(batch, dev)
    assert plan.rel_total >= 1024

    def data(seed):
        rng = np.random.default_rng(seed)
        return [(0.3 * rng.standard_normal((cfg.R1, D))).astype(np.float32), (0.3 * rng.standard_normal((cfg.R1, D))).astype(np.float32),
                (0.3 * rng.standard_normal((B, I, D))).astype(np.float32),
                rng.uniform(-0.05, 0.05, size=(D, (2 * I + 1) * D)).astype(np.float32),
                (rng.standard_normal((D, D)) / np.sqrt(D) * 0.4).astype(np.float32), (0.1 * rng.standard_normal(D)).astype(np.float32)]

    def call(rf, rfi, ins, W, Wr, br):
        T, planes = ops.rel_transform(rf, rfi, [(Wr, br, None, None)], planes=True)
        return (T, ops.relation_tables(plan, T[0, 0], T[0, 1], ins, W, math=ops.MATH_BF16X3),
                ops.relation_tables_planes(plan, planes[0], ins, W),
                ops.relation_tables(plan, T[0, 0], T[0, 1], ins, W, math=ops.MATH_FP32))

    d0, d1 = data(5), data(6)
    runs = _three(g, call, _t(dev, *d0), _t(dev, *d1))
    for run in runs:
        T = run[0].numpy()
        want = _tables_f64(plan, dict(T_f=T[0, 0], T_i=T[0, 1], ins=d0[2], W=d0[3]), cfg)
        for k in (1, 2, 3):
            assert np.abs(run[k].numpy() - want).max() <= TOL_KERNEL * max(1.0, np.abs(want).max()), k


@pytest.mark.parametrize("gather", [True, False], ids=["gather", "lds"])
@pytest.mark.parametrize("name", GRAPH_CASES)
def test_backward_kernels(dev, g, name, gather):
    """gnnrag_aggregate_backward, gnnrag_typelayer_backward (gather and LDS-atomic forms), gnnrag_aggregate_fused_backward
    and the ordering they read (gnnrag_relorder_build, rebuilt under every fill): float64 autograd / sums within 2e-5 of
    the largest entry under every fill; the gather forms at D % 4 == 0 and the fused backward bit-identical."""
    import oracle.rearev_grad as og
    from gnnrag_amd import ops, synth
    cfg = _cfg(name)
    batch = synth.make_batch(cfg)
    et = batch.edge_tuple
    B, N, D, I = cfg.B, cfg.N, cfg.D, cfg.I
    plan = _plan(batch, dev)
    plan.attach_w_rel(et[6])
    fused_bwd = D % 4 == 0 and gather
    d0, d1 = _layer_data(cfg, 17), _layer_data(cfg, 18)
    P0 = [(0.3 * np.random.default_rng(s).standard_normal((2, plan.rel_total, D))).astype(np.float32) for s in (1, 2)]
    keys = ("dist", "ins", "T_f", "T_i", "g_agg", "g_nbr")

    def call(dist, ins, T_f, T_i, g_agg, g_nbr, P):
        out = ops.aggregate_backward(plan, dist, ins, T_f, T_i, g_agg, gather=gather)
        out += (ops.typelayer_backward(plan, g_nbr, False, gather=gather), ops.typelayer_backward(plan, g_nbr, True, gather=gather))
        if fused_bwd:
            out += ops.aggregate_fused_backward(plan, dist, P, g_nbr)
        return out

    runs = _three(g, call, _t(dev, *[d0[k] for k in keys], P0[0]), _t(dev, *[d1[k] for k in keys], P0[1]),
                  lambda: _drop_workspaces(plan, relorder=True))
    weight = et[5] if cfg.normalized_gnn else None
    want = list(og.aggregate_grads(et, B, N, d0["dist"], d0["ins"], d0["T_f"], d0["T_i"], d0["g_agg"], weight)[1:])
    want += [og.typelayer_grad(et, B, N, d0["T_f"], d0["g_nbr"], None), og.typelayer_grad(et, B, N, d0["T_f"], d0["g_nbr"], et[6])]
    if fused_bwd:
        _, (h, t, w, row_of, d64, P64) = _walk_f64(plan, batch, d0["dist"], P0[0])
        g64 = d0["g_nbr"].astype(np.float64)
        gd = np.zeros(B * N)
        np.add.at(gd, h, w * np.einsum("fd,fd->f", g64[t], P64[0][row_of]))
        np.add.at(gd, t, w * np.einsum("fd,fd->f", g64[h], P64[1][row_of]))
        gP = np.zeros_like(P64)
        np.add.at(gP[0], row_of, (w * d64[h])[:, None] * g64[t])
        np.add.at(gP[1], row_of, (w * d64[t])[:, None] * g64[h])
        want += [gd, gP]
    names = ["g_dist", "g_ins", "g_T_fwd", "g_T_inv", "g_T", "g_T (w_rel)", "fused g_dist", "fused g_P"]
    for run in runs:
        for k, wv in enumerate(want):
            _close(run[k], wv.reshape(run[k].shape), TOL_KERNEL, names[k])
    if gather and D % 4 == 0:
        _bit_identical(runs, _plain(g, lambda: call(*_t(dev, *[d0[k] for k in keys], P0[0]))), "backward")


def test_empty_batch(dev, g):
    """No facts at all (test_empty_batch_backward): every output is written (zeros), whatever the buffers held.  The fused
    walk and its backward are left out: with rel_total == 0 the table P [2, 0, D] has no address and the library refuses
    a null pointer (GNNRAG_E_BADARG), so the caller-zeroed g_P of that case never reaches a kernel."""
    from gnnrag_amd import ops
    z = np.zeros(0, np.int64)
    plan = ops.CsrPlan(z, z, z, 2, 8, 3, dev)
    D, I = 16, 2
    gen = torch.Generator().manual_seed(0)
    inp = [torch.full((2, 8), 0.125), torch.randn(2, I, D, generator=gen), torch.randn(3, D, generator=gen),
           torch.randn(16, 2 * I * D, generator=gen), torch.randn(16, D, generator=gen)]

    def call(dist, ins, T, gagg, gn):
        return (ops.aggregate(plan, dist, ins, T, T), ops.typelayer(plan, T, False)) + \
            ops.aggregate_backward(plan, dist, ins, T, T, gagg) + (ops.typelayer_backward(plan, gn, False),)

    runs = _three(g, call, [x.to(dev) for x in inp], [x.to(dev) for x in inp], lambda: _drop_workspaces(plan, relorder=True))
    for run in runs:
        for k, o in enumerate(run):
            assert not o.numpy().any() and np.isfinite(o.numpy()).all(), k


@pytest.mark.parametrize("case", ["one_seed", "three_seeds", "hub_seed", "weighted", "bn_plus1"])
def test_frontier_trio(dev, g, case):
    """gnnrag_frontier_build / gnnrag_relation_tables_frontier / gnnrag_aggregate_fused_frontier: the lists beyond their
    counts are unspecified (gnnrag.h: "lists both"; only the counts and the row gates are read back), so the row gates,
    the counts and the LISTED rows of P / out are compared; unlisted rows keep what the caller put there (gnnrag.h:
    "every other row of `out` is left untouched") - NaN for P, the caller's zeros for out - under every fill."""
    from gnnrag_amd import ops, synth
    from test_gpu_frontier import _cfg as fcfg, _numpy_frontier
    cfg = _cfg("bn_plus1") if case == "bn_plus1" else fcfg(**(dict(normalized_gnn=True) if case == "weighted" else {}))
    batch = synth.make_batch(cfg)
    plan = _plan(batch, dev)
    rng = np.random.default_rng(5)
    dist = batch.seed_dist.astype(np.float32).copy()
    if case == "three_seeds":
        for b in range(cfg.B):
            dist[b] = 0
            dist[b, rng.choice(cfg.N, 3, replace=False)] = 1.0 / 3
    elif case == "hub_seed":
        dist[:] = 0
        dist[:, 1] = 1.0
    other = np.roll(dist, 7, axis=1)
    d0, d1 = _layer_data(cfg, 3), _layer_data(cfg, 4)
    keys = ("ins", "T_f", "T_i", "W")

    def call(dd, ins, T_f, T_i, W):
        fr = ops.Frontier(plan, dd)
        nrows, ntrows, flags = fr.read()
        P = fr.relation_tables(T_f, T_i, ins, W)
        listed = ~torch.isnan(P[0, :, 0])
        nbr = fr.aggregate(torch.where(torch.isnan(P), torch.zeros_like(P), P))
        return torch.tensor([nrows, ntrows]), torch.from_numpy(flags), listed, P, nbr

    runs = _three(g, call, _t(dev, dist, *[d0[k] for k in keys]), _t(dev, other, *[d1[k] for k in keys]))
    want_flags, want_pairs = _numpy_frontier(batch, dist)
    want_P = _tables_f64(plan, d0, cfg)
    for run in runs:
        counts, flags, listed, P, nbr = run
        assert np.array_equal(flags.numpy(), want_flags) and counts.tolist() == [int(want_flags.sum()), want_pairs]
        assert int(listed.sum()) == want_pairs and torch.isnan(P[:, ~listed]).all()
        Pl = P[:, listed].numpy()
        assert np.abs(Pl - want_P[:, listed.numpy()]).max() <= TOL_KERNEL * max(1.0, np.abs(want_P).max())
        Pz = torch.where(torch.isnan(P), torch.zeros_like(P), P).numpy()
        want_nbr, _ = _walk_f64(plan, batch, dist, Pz)
        on = want_flags.astype(bool)
        assert not nbr.numpy()[~on].any()
        assert np.abs(nbr.numpy() - want_nbr).max() <= TOL_KERNEL * max(1.0, np.abs(want_nbr).max())
    for k in (0, 1, 2):
        _bit_identical([[r[k]] for r in runs], None, "frontier lists")


# -- whole layers --------------------------------------------------------------------------------------------------------

def _layer_inputs(cfg, batch, seed):
    from gnnrag_amd import synth
    feats = synth.make_features(cfg, seed=seed)
    params = synth.make_layer_params(cfg, seed=seed)
    mask = (batch.local_entity != batch.num_entity).astype(np.float32)
    rng = np.random.default_rng(seed)
    dense = rng.random((cfg.B, cfg.N)).astype(np.float32)
    dense /= dense.sum(1, keepdims=True)
    names = ["rel_linear0.weight", "rel_linear0.bias", "e2e_linear0.weight", "e2e_linear0.bias", "score_func.weight",
             "score_func.bias"]
    arrs = [feats["h0"], dense, feats["ins"][0], feats["rel_features"], feats["rel_features_inv"]] + [params[n] for n in names] + [mask]
    if cfg.pos_emb:
        arrs += [params["pos_emb0.weight"], params["pos_emb_inv0.weight"]]
    return feats, params, mask, dense, arrs


@pytest.mark.parametrize("path", [1, 2], ids=["unfused", "fused"])
@pytest.mark.parametrize("name", ["tiny", "tiny50", "tinyfb", "hub", "huge", "odd", "bn_plus1", "bn_minus1", "not512"])
def test_reason_layer(dev, g, name, path):
    """gnnrag_reason_layer on both kernel paths with a workspace object kept across the calls (ops.LayerWorkspace keeps one
    grown buffer: the second and third call really run in the first one's leftovers; a fresh one gets the 0xFF fill):
    float64 oracle within the tolerances of a layer call in test_gpu_random_sweep.py, bit-identical under every fill."""
    import oracle.rearev_np64 as onp
    from gnnrag_amd import ops, synth
    cfg = _cfg(name)
    batch = synth.make_batch(cfg)
    plan = _plan(batch, dev)
    B, N, D = cfg.B, cfg.N, cfg.D
    feats, params, mask, dense, a0 = _layer_inputs(cfg, batch, 31)
    a1 = _layer_inputs(cfg, batch, 32)[4]
    kept = ops.LayerWorkspace()

    def call(h, dist, ins, rf, rfi, Wr, br, We, be, ws, bs, mk, pos=None, posi=None):
        w = ops.LayerWorkspace() if g.fill == FILL_ONES else kept
        return ops.reason_layer(plan, h, dist, ins, rf, rfi, Wr, br, We, be, ws, bs, mk, pos, posi, ws=w, path=path)

    runs = _three(g, call, _f32(dev, *a0), _f32(dev, *a1), lambda: _drop_workspaces(plan))
    score, nd, hn, _ = onp.layer_call(batch.edge_tuple, B, N, feats["h0"], mask, dense, feats["ins"][0], params, 0,
                                      feats["rel_features"], feats["rel_features_inv"],
                                      normalized_gnn=cfg.normalized_gnn, use_posemb=cfg.pos_emb)
    valid = mask.reshape(-1) > 0
    h_out, sc, dist_out = (x.numpy() for x in runs[0])
    # tolerances of a layer call in test_gpu_random_sweep.py (rtol 5e-6: unnormalised hub sums reach 10^2; atol 2e-5)
    np.testing.assert_allclose(h_out.reshape(B * N, D), hn.reshape(B * N, D), rtol=5e-6, atol=TOL_KERNEL)
    np.testing.assert_allclose(sc.reshape(-1)[valid], score.reshape(-1)[valid], rtol=5e-6, atol=TOL_KERNEL)
    assert (sc.reshape(-1)[~valid] == np.float32(-1e11)).all()
    np.testing.assert_allclose(dist_out, nd, rtol=5e-6, atol=TOL_KERNEL)
    _bit_identical(runs, _plain(g, lambda: ops.reason_layer(plan, *_f32(dev, *a0[:12]), *_f32(dev, *a0[12:]), path=path)),
                   "reason_layer")


def test_layer_workspace_kept_across_shapes(dev, g):
    """ops.LayerWorkspace keeps ONE grown buffer across batches of different shapes (the module holds one per layer
    object): a large batch, then a small one in the large one's leftovers, then the large one again in the small one's -
    each bit-identical to the same call with a workspace of its own (0x00 and 0xFF filled), on both kernel paths."""
    from gnnrag_amd import ops, synth
    kept = {1: ops.LayerWorkspace(), 2: ops.LayerWorkspace()}
    for step, name in enumerate(["hub", "tiny", "bn_plus1", "hub", "tiny50", "not512"]):
        cfg = _cfg(name)
        batch = synth.make_batch(cfg)
        plan = _plan(batch, dev)
        args = [g.wrap(t, "input %d" % i) for i, t in enumerate(_f32(dev, *_layer_inputs(cfg, batch, 40 + step)[4]))]
        for path in (1, 2):
            outs = []
            for fill, ws in ((FILL_ZERO, None), (FILL_ONES, None), (FILL_ONES, kept[path])):
                g.fill = fill
                _drop_workspaces(plan)
                outs.append(_snap(ops.reason_layer(plan, *args[:12], *args[12:], ws=ws, path=path)))
                g.check("%s, path %d, %s workspace" % (name, path, "kept" if ws else "own"))
            _bit_identical(outs, None, "%s path %d" % (name, path))
    assert kept[1].buf is not None and kept[2].buf is not None


def _module_run(cfg, batch, feats, params, dev, path, type_layer=False):
    from gnnrag_amd import stack
    return stack.run_stack(batch, feats, params, dev, use_type_layer=type_layer, norm_rel=cfg.normalized_gnn and type_layer,
                           path=path)


def _module_three(g, run):
    """A whole module forward (structure build, TypeLayer, gnnrag_reason_stack / gnnrag_reason_layer per the module's
    switches) with every buffer of the binding guarded, under 0x00, leftovers of the previous forward, 0xFF."""
    outs = []
    for fill in (FILL_ZERO, FILL_LEFTOVERS, FILL_ONES):
        g.fill = fill
        outs.append(run())
        g.check("module forward, body fill %r" % (fill,))
    return outs


def _module_equal(outs, plain, cfg):
    for k, o in enumerate(outs[1:] + [plain]):
        for key in ("h", "score", "dist"):
            for c in range(cfg.T * cfg.L):
                assert np.array_equal(outs[0][key][c], o[key][c]), "%s[%d] differs in run %d" % (key, c, k + 1)
        if "h0" in o:
            assert np.array_equal(outs[0]["h0"], o["h0"])


@pytest.mark.parametrize("path", [1, 2], ids=["unfused", "fused"])
@pytest.mark.parametrize("k", [0, 1, 2, 3, 5, 6, 7, 9, 12, 21])
def test_random_sweep_cases_guarded(dev, g, k, path):
    """Seeded cases of test_gpu_random_sweep._random_cfg (odd N / D / I, questions without facts, duplicate facts, every
    vocabulary size) through the module's forward - TypeLayer, structure build, the whole-iteration call - against the
    float64 oracle with that test's tolerances, and bit-identical under every fill."""
    import oracle.rearev_np64 as onp
    from gnnrag_amd import synth
    from test_gpu_random_sweep import RTOL, TOL, _random_cfg
    rng = np.random.default_rng(1000 + k)
    cfg = _random_cfg(rng, k)
    batch = synth.make_batch(cfg)
    feats = synth.make_features(cfg)
    params = synth.make_layer_params(cfg)
    want = onp.run_stack(batch, feats, params, use_type_layer=True, norm_rel=cfg.normalized_gnn)
    outs = _module_three(g, lambda: _module_run(cfg, batch, feats, params, dev, path, True))
    got = outs[0]
    np.testing.assert_allclose(got["h0"], want["h0"], rtol=RTOL, atol=TOL)
    for c in range(cfg.T * cfg.L):
        np.testing.assert_allclose(got["h"][c], want["h"][c], rtol=RTOL, atol=TOL, err_msg="%s h %d" % (cfg, c))
        np.testing.assert_allclose(got["dist"][c], want["dist"][c], rtol=RTOL, atol=TOL, err_msg="%s dist %d" % (cfg, c))
    _module_equal(outs, _plain_module(g, lambda: _module_run(cfg, batch, feats, params, dev, path, True)), cfg)


def _plain_module(g, fn):
    from gnnrag_amd import ops
    saved, ops._buf = ops._buf, g.plain
    try:
        return fn()
    finally:
        ops._buf = saved


@pytest.mark.parametrize("path", [2, 1], ids=["fused", "unfused"])
def test_large_ragged_shape_guarded(dev, g, path):
    """test_random_large_shape case 0 (W-resident bf16x3 tables and update in the default math mode, ragged node count):
    float64 oracle with its tolerances, bit-identical under every fill."""
    import oracle.rearev_np64 as onp
    from gnnrag_amd import synth
    from test_gpu_random_sweep import TOL
    rng = np.random.default_rng(7000)
    N = int(rng.integers(900, 2300))
    B = int(rng.integers(max(4, 8192 // N + 1), 14))
    used = int(rng.integers(150, 500)) if rng.integers(0, 2) else None
    cfg = synth.GraphConfig(name="large0", B=B, N=N, E=int(rng.integers(3 * N, 7 * N)),
                            R=int(rng.choice([300, 650, 3000])) if used is None else 3000, D=int(rng.choice([200, 208])),
                            I=int(rng.integers(1, 4)), L=2, T=1, seed=int(rng.integers(1, 10 ** 6)),
                            zipf_heads=bool(rng.integers(0, 2)), normalized_gnn=bool(rng.integers(0, 2)),
                            pos_emb=bool(rng.integers(0, 2)), n_real_min=N // 2, rel_per_question=used)
    batch = synth.make_batch(cfg)
    feats = synth.make_features(cfg)
    params = synth.make_layer_params(cfg)
    want = onp.run_stack(batch, feats, params, use_type_layer=False)
    outs = _module_three(g, lambda: _module_run(cfg, batch, feats, params, dev, path))
    for c in range(cfg.T * cfg.L):
        scale = max(1.0, float(np.abs(want["h"][c]).max()))
        np.testing.assert_allclose(outs[0]["h"][c], want["h"][c], rtol=0, atol=TOL * scale)
        np.testing.assert_allclose(outs[0]["dist"][c], want["dist"][c], rtol=0, atol=TOL)
    _module_equal(outs, _plain_module(g, lambda: _module_run(cfg, batch, feats, params, dev, path)), cfg)


@pytest.mark.parametrize("path", [1, 2], ids=["unfused", "fused"])
def test_c2_forward_guarded(dev, g, path):
    """BASELINE config C2 at full size (the XCD mapping and the ticketed work lists only engage at full grids), once per
    forward path: guards hold and the forward is bit-identical under 0x00 / leftovers / 0xFF and to the unguarded run,
    whose values test_full_size_properties_c2 and the fixtures pin (no float64 oracle at this size there either); the
    size-independent properties of that test are asserted on the guarded result."""
    from gnnrag_amd import synth
    cfg = synth.CONFIGS["C2"]
    batch = synth.make_batch(cfg)
    feats = synth.make_features(cfg)
    params = synth.make_layer_params(cfg)
    outs = _module_three(g, lambda: _module_run(cfg, batch, feats, params, dev, path))
    d = outs[0]["dist"][-1]
    mask = batch.local_entity != batch.num_entity
    np.testing.assert_allclose(d.sum(1), 1.0, atol=1e-5)
    assert (d[~mask] == 0).all() and np.isfinite(d).all()
    _module_equal(outs, _plain_module(g, lambda: _module_run(cfg, batch, feats, params, dev, path)), cfg)


def _explicit_stack(layer, cfg, devin):
    """The module's own LayerStack operands (test_whole_iteration_call_and_graph_replay_are_bit_identical)."""
    import torch.nn.functional as F
    from gnnrag_amd import ops
    P = layer._inference_params()
    D, Dp = P["D"], P["Dp"]
    pad = (lambda t: t if Dp == D else F.pad(t, (0, Dp - D)))
    st = ops.LayerStack(layer.plan, P["relfeat"], P["relfeat_inv"], P["layers"], P["w_score"], P["b_score"],
                        layer.local_entity_mask, cfg.I, path=layer._path_of(0))
    return st, pad, D


@pytest.mark.parametrize("cfgname", ["tiny50", "mid", "bn_plus1"])
def test_layer_stack_run_capture_replay(dev, g, cfgname):
    """gnnrag_reason_stack, gnnrag_reason_stack_capture and gnnrag_graph_launch with guarded outputs and workspace: the
    eager run is bit-identical under every fill and equals the per-layer calls; a captured graph replayed three times
    equals the eager sequence bit for bit and the guards hold after the replays."""
    from gnnrag_amd import stack, synth
    if cfgname == "mid":
        cfg = synth.GraphConfig(name="mid", B=4, N=2000, E=10000, R=600, D=200, I=2, L=3, T=3, seed=21)
    elif cfgname == "tiny50":
        cfg = synth.GraphConfig(**{**synth.CONFIGS["tiny50"].__dict__, "T": 3})
    else:
        cfg = dataclasses.replace(_cfg(cfgname), T=3)
    batch = synth.make_batch(cfg)
    feats = synth.make_features(cfg)
    params = synth.make_layer_params(cfg)
    devin = stack.DeviceInputs(batch, feats, dev)
    layer = stack.build_layer(cfg, batch, params, dev)
    layer.use_stack = False
    stack.init_reason(layer, batch, devin, devin.h0)
    _, per_layer = stack.run_layers(layer, cfg, devin, record=True)
    g.check("per-layer calls")
    with torch.no_grad():
        eager = []
        for fill in (FILL_ZERO, FILL_LEFTOVERS, FILL_ONES):
            g.fill = fill
            layer = stack.build_layer(cfg, batch, params, dev)
            stack.init_reason(layer, batch, devin, devin.h0)
            st, pad, D = _explicit_stack(layer, cfg, devin)
            h_prev, rec = pad(devin.h0), []
            for t in range(cfg.T):
                h, score, dist = st.run(h_prev, devin.seed_dist, pad(devin.ins[t]))
                rec.append(_snap((h, score, dist)))
                h_prev = h[cfg.L - 1]
            g.check("LayerStack.run, body fill %r" % (fill,))
            eager.append([x for r in rec for x in r])
        _bit_identical(eager, None, "LayerStack.run")
        c = 0
        for t in range(cfg.T):
            for j in range(cfg.L):
                assert np.array_equal(eager[0][3 * t][j][..., :D].numpy(), per_layer["h"][c])
                assert np.array_equal(eager[0][3 * t + 1][j].numpy(), per_layer["score"][c])
                assert np.array_equal(eager[0][3 * t + 2][j].numpy(), per_layer["dist"][c])
                c += 1
        # the captured form in 0xFF-filled fixed buffers (st is the stack of the last fill; its eager runs happened above)
        st.new_forward()
        ins_buf = g.wrap(pad(devin.ins[0]), "capture: ins")
        g.blocks[-1].copy = None                                   # rewritten in place between replays, by the test
        st.run(pad(devin.h0), devin.seed_dist, ins_buf)
        st.capture(pad(devin.h0), devin.seed_dist, ins_buf)
        c = 0
        for t in range(cfg.T):
            ins_buf.copy_(pad(devin.ins[t]))
            h, score, dist = st.replay(first=(t == 0))
            g.check("replay %d" % t)
            for j in range(cfg.L):
                assert np.array_equal(h[j][..., :D].cpu().numpy(), per_layer["h"][c])
                assert (h[j][..., D:] == 0).all()
                assert np.array_equal(dist[j].cpu().numpy(), per_layer["dist"][c])
                assert np.array_equal(score[j].cpu().numpy(), per_layer["score"][c])
                c += 1
        st.release_graph()
    assert cfg.T >= 3


# -- paths ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,B,seed", [("C1", 1, 3), ("C3", 32, 5), ("tiny", 3, 7)])
def test_selection_and_shortest_paths(dev, g, shape, B, seed):
    """gnnrag_topp_candidates_ws -> gnnrag_shortest_paths with guarded outputs and workspace.  The records behind
    path_off[P] are unspecified (gnnrag.h: "path_off[P] of them exist, the rest of the two arrays is not touched"), so
    only the first path_off[-1] records are compared (test_gpu_paths._host); the rest against tests/paths_oracle.py."""
    import paths_oracle
    from gnnrag_amd import ops, synth
    from test_gpu_paths import _check_against_oracle, _host, _peaked_pred
    cfg = dataclasses.replace(synth.CONFIGS[shape], B=B)
    batch = synth.make_batch(cfg, seed=seed)
    h, r, t = batch.edge_tuple[:3]
    N = cfg.N
    graph = ops.UGraph.from_plan(ops.CsrPlan(h, r, t, B, N, cfg.R1, dev))
    seeds = batch.query_entities == 1
    eligible = ((~seeds) & (batch.local_entity != batch.num_entity)).astype(np.uint8)
    S, C, K, H = 2, 16, 64, 16
    eps = 0.95

    def call(pred, el, sf):
        slots, cnt = ops.topp_candidates(pred, el, (1 - eps) / N, eps)
        out = _host(ops.shortest_paths(graph, sf, slots, cnt, S, C, K, H, buffers=ops.PathBuffers(B, N, S, C, K, H, dev)))
        return [slots, cnt] + [torch.from_numpy(out[k]) for k in ("q_info", "pair_info", "path_off", "nodes", "facts")]

    p0 = _peaked_pred(np.random.default_rng(100 + seed), batch)
    p1 = _peaked_pred(np.random.default_rng(200 + seed), batch)
    sf = seeds.astype(np.uint8)
    runs = _three(g, call, _t(dev, p0, eligible, sf), _t(dev, p1, eligible, sf))
    slots_h, cnt_h = runs[0][0].numpy(), runs[0][1].numpy()
    want = paths_oracle.batch(h, t, B, N, seeds, slots_h, cnt_h, S, C, K, H)
    got = dict(zip(("q_info", "pair_info", "path_off", "nodes", "facts"), (x.numpy() for x in runs[0][2:])))
    _check_against_oracle(got, want, S, C, H)
    _bit_identical(runs, _plain(g, lambda: call(*_t(dev, p0, eligible, sf))), "paths")


# -- stated sizes ----------------------------------------------------------------------------------------------------------

def _refused(fn):
    """None when the call was refused with GNNRAG_E_WORKSPACE, else what happened instead."""
    from gnnrag_amd import _lib
    try:
        fn()
    except _lib.GnnragError as e:
        m = re.search(r"failed \((-?\d+)\)", str(e))
        return None if m and int(m.group(1)) == E_WORKSPACE else str(e)
    return "accepted"


def test_stated_sizes_are_sufficient_and_enforced(dev, g):
    """Every entry point that takes a byte count (gnnrag_aggregate_fused_hub_form excepted: gnnrag.h states no size for
    it, what it reports is a function of the size it is given): with exactly gnnrag_*_bytes(...) (the binding passes the buffer's size;
    asserted > the 256-byte floor, so it IS the stated size) the call succeeds with intact guards - that is every other
    test of this file - and with one byte less it returns GNNRAG_E_WORKSPACE.  The memory stays whole in both calls
    (``Guard.short`` only shrinks the size the binding sees and passes on), so nothing can run out of bounds."""
    import ctypes as C
    from gnnrag_amd import _lib, ops, synth
    lib = _lib.load()
    cfg = _cfg("hub")
    batch = synth.make_batch(cfg)
    et = batch.edge_tuple
    B, N, D, I = cfg.B, cfg.N, cfg.D, cfg.I
    d = {k: v for k, v in zip(("dist", "ins", "T_f", "T_i", "W", "g_agg", "g_nbr"),
                              _t(dev, *[_layer_data(cfg, 1)[k] for k in ("dist", "ins", "T_f", "T_i", "W", "g_agg", "g_nbr")]))}
    hrt = torch.from_numpy(np.stack([np.asarray(et[k]) for k in range(3)]).astype(np.int32)).to(dev)
    F = hrt.shape[1]

    def build():
        return ops.CsrPlan(None, None, None, B, N, cfg.R1, dev, hrt_device=hrt)

    plan = build()
    parts = []
    for b in range(B):
        sub = hrt[:, (hrt[0] // N) == b].clone()
        sub[0] -= b * N
        sub[2] -= b * N
        parts.append(ops.CsrPlan(None, None, None, 1, N, cfg.R1, dev, hrt_device=sub.contiguous()))
    g.sizes.clear()
    plan = build()
    assert g.sizes["csr_build: csr_mem"] == lib.gnnrag_csr_bytes(F, B, N, cfg.R1, 0, 0) > 256
    assert g.sizes["csr_build: scratch"] == lib.gnnrag_csr_scratch_bytes(F, B, N, cfg.R1) > 256
    P = ops.relation_tables(plan, d["T_f"], d["T_i"], d["ins"], d["W"])
    feats, params, mask, dense, arrs = _layer_inputs(cfg, batch, 31)
    la = _f32(dev, *arrs)
    pred = torch.rand(2, 20000, device=dev)
    el = torch.ones(2, 20000, dtype=torch.uint8, device=dev)
    x, wi, wh = torch.randn(3, 4, 64, device=dev), torch.randn(4 * 32, 64, device=dev), torch.randn(4 * 32, 32, device=dev)
    A, Bm = torch.randn(5000, 56, device=dev), torch.randn(5000, 56, device=dev)
    ug = ops.UGraph(plan)
    sf = torch.from_numpy((batch.query_entities == 1).astype(np.uint8)).to(dev)
    slots, cnt = ops.topp_candidates(torch.rand(B, N, device=dev), torch.ones(B, N, dtype=torch.uint8, device=dev), 0.0, 0.9)
    layers = [(la[5], la[6], la[7], la[8], None, None)] * 2

    def stack_run():
        st = ops.LayerStack(plan, la[3], la[4], layers, la[9], la[10], la[11], I)
        return st.run(la[0], la[1], la[2])

    def fresh(fn, relorder=False):
        def run():
            _drop_workspaces(plan, relorder=relorder)
            return fn()
        return run

    calls = [   # (role of the sized buffer, the call)
        ("csr_build: csr_mem", build), ("csr_build: scratch", build),
        ("csr_concat: csr_mem", lambda: ops.CsrPlan.concat(parts, N, cfg.R1, dev)),
        ("aggregate / typelayer: workspace", fresh(lambda: ops.aggregate(plan, d["dist"], d["ins"], d["T_f"], d["T_i"]))),
        ("aggregate / typelayer: workspace", fresh(lambda: ops.aggregate_fused(plan, d["dist"], P))),
        ("aggregate / typelayer: workspace", fresh(lambda: ops.typelayer(plan, d["T_f"], False))),
        ("relorder_build: mem", fresh(plan.relorder, True)), ("relorder_build: scratch", fresh(plan.relorder, True)),
        ("backward: workspace", fresh(lambda: ops.aggregate_backward(plan, d["dist"], d["ins"], d["T_f"], d["T_i"], d["g_agg"]))),
        ("backward: workspace", fresh(lambda: ops.aggregate_backward(plan, d["dist"], d["ins"], d["T_f"], d["T_i"], d["g_agg"], gather=False))),
        ("backward: workspace", fresh(lambda: ops.aggregate_fused_backward(plan, d["dist"], P, d["g_nbr"]))),
        ("backward: workspace", fresh(lambda: ops.typelayer_backward(plan, d["g_nbr"], False))),
        ("backward: workspace", fresh(lambda: ops.typelayer_backward(plan, d["g_nbr"], False, gather=False))),
        ("gemm_tn: workspace", lambda: ops.gemm_tn(A, Bm)),
        ("reason_layer: workspace", lambda: ops.reason_layer(plan, *la[:12], path=1)),
        ("reason_layer: workspace", lambda: ops.reason_layer(plan, *la[:12], path=2)),
        ("frontier_build: fws", lambda: ops.Frontier(plan, d["dist"])),
        ("topp_candidates_ws: workspace", lambda: ops.topp_candidates(pred, el, 0.0, 0.9)),
        ("lstm_forward: workspace", lambda: ops.lstm_forward(x, wi, wh)),
        ("ugraph_build: mem", lambda: ops.UGraph(plan)), ("ugraph_build: scratch", lambda: ops.UGraph(plan)),
        ("shortest_paths: workspace", lambda: ops.shortest_paths(ug, sf, slots, cnt, 2, 16, 64, 8,
                                                                 buffers=ops.PathBuffers(B, N, 2, 16, 64, 8, dev))),
    ]
    floors = {"gemm_tn: workspace": 16, "topp_candidates_ws: workspace": 16, "lstm_forward: workspace": 0,
              "ugraph_build: mem": 0, "ugraph_build: scratch": 0, "shortest_paths: workspace": 0}
    wrong = []
    for k, (role, fn) in enumerate(calls):
        g.short = {}
        fn()                                                    # the stated size: accepted
        g.check("%s at its stated size" % role)
        assert g.sizes[role] > floors.get(role, 256), (role, g.sizes[role])     # above the binding's floor: the exact size
        g.short = {role: 1}
        got = _refused(fn)                                      # one byte less: refused, nothing launched
        if got is not None:
            wrong.append("call %d, %s one byte short: %s" % (k, role, got))
        g.check("%s one byte short" % role)
    g.short = {}
    assert not wrong, "\n".join(wrong)
    # gnnrag_reason_stack: gnnrag_stack_workspace_bytes buys the up-front projections; the stated minimum is
    # gnnrag_layer_workspace_bytes ("the stack call still works and projects per layer (same results bit for bit)")
    role = "reason_stack: workspace"
    full = _snap(stack_run())
    big, small = g.sizes[role], lib.gnnrag_layer_workspace_bytes(C.byref(plan.c), D, I)
    assert big == lib.gnnrag_stack_workspace_bytes(C.byref(plan.c), 2, D, I) > small > 256
    g.short = {role: big - small}
    _bit_identical([full, _snap(stack_run())], None, "reason_stack with the layer-sized workspace")
    g.check("%s at gnnrag_layer_workspace_bytes" % role)
    g.short = {role: big - small + 1}
    assert _refused(stack_run) is None
    g.check("%s one byte short" % role)
    g.short = {}
    _drop_workspaces(plan, relorder=True)


# -- streams ---------------------------------------------------------------------------------------------------------------

def test_side_stream_calls_are_bit_identical(dev, g):
    """Forward (gnnrag_reason_layer on both paths, LayerStack.run), gnnrag_aggregate_fused, the gather backward, the
    structure build (waiting and deferred form), gnnrag_lstm_forward and gnnrag_query_reform on a side stream, an input
    of each produced there by a torch op right before the call and nothing waited for in between: bit-identical to the
    default-stream call, guards intact."""
    from gnnrag_amd import ops, synth
    cfg = _cfg("hub")
    batch = synth.make_batch(cfg)
    et = batch.edge_tuple
    B, N, D, I = cfg.B, cfg.N, cfg.D, cfg.I
    hrt = torch.from_numpy(np.stack([np.asarray(et[k]) for k in range(3)]).astype(np.int32)).to(dev)
    pairs = np.unique(np.stack([np.asarray(et[0]) // N, np.asarray(et[1])], 1), axis=0)
    per_q = np.bincount(pairs[:, 0], minlength=B)
    plan = ops.CsrPlan(None, None, None, B, N, cfg.R1, dev, hrt_device=hrt)
    d = _layer_data(cfg, 1)
    raw, ins, T_f, T_i, W, g_agg, g_nbr = _t(dev, d["dist"] * 3.0, d["ins"], d["T_f"], d["T_i"], d["W"], d["g_agg"], d["g_nbr"])
    la = _f32(dev, *_layer_inputs(cfg, batch, 31)[4])
    layers = [(la[5], la[6], la[7], la[8], None, None)] * 2
    gen = torch.Generator().manual_seed(1)
    x, wi, wh = (torch.randn(*s, generator=gen).to(dev) for s in ((5, 6, 64), (128, 64), (128, 32)))
    q, Wr, Wg = (torch.randn(*s, generator=gen).to(dev) / 8 for s in ((B, D), (D, 3 * D), (D, 3 * D)))
    ent = torch.randn(B, N, D, generator=gen).to(dev)

    def everything():
        dist = raw / raw.sum(1, keepdim=True)                    # the torch op right before the calls, on this stream
        P = ops.relation_tables(plan, T_f, T_i, ins, W)
        out = list(ops.reason_layer(plan, la[0], dist, *la[2:12], path=1))
        out += ops.reason_layer(plan, la[0], dist, *la[2:12], path=2)
        out += ops.LayerStack(plan, la[3], la[4], layers, la[9], la[10], la[11], I).run(la[0], dist, la[2])
        out.append(ops.aggregate_fused(plan, dist, P))
        out += ops.aggregate_backward(plan, dist, ins, T_f, T_i, g_agg)
        out += ops.aggregate_fused_backward(plan, dist, P, g_nbr)
        ids = hrt + 0                                            # produced on this stream as well
        for rc in (None, (int(per_q.sum()), int(per_q.max()))):
            p2 = ops.CsrPlan(None, None, None, B, N, cfg.R1, dev, hrt_device=ids, rel_counts=rc)
            out.append(ops.aggregate_fused(p2, dist, P))
            keep.append(p2)
        out += ops.lstm_forward(x * 1.5, wi, wh)
        out.append(ops.query_reform(q, dist, ent * 0.5, Wr, Wg))
        return out

    keep = []
    want = _snap(everything())
    g.check("default stream")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _drop_workspaces(plan, relorder=True)
        got = everything()
    side.synchronize()
    g.check("side stream")
    got = _snap(got)
    _bit_identical([want, got], None, "side stream")
