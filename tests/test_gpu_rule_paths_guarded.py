"""gnnrag_rule_paths between guard bytes (tests/guarded.py, as tests/test_gpu_guarded.py uses it): every output and the
workspace are exact-sized views with guards on both sides, their bodies pre-filled with 0x00, with what a call on other
inputs left behind, and with 0xFF.  The results must be bit-identical across the fills and equal the restatement, no guard
byte may change, and a workspace one byte below the stated size is refused before anything is launched."""
import ctypes as C

import numpy as np
import pytest
import torch

import guarded
import rule_paths_oracle
from guarded import FILL_LEFTOVERS, FILL_ONES, FILL_ZERO

pytestmark = pytest.mark.gpu
E_WORKSPACE = -3
ROLES = ["rule_paths: q_info", "rule_paths: pair_info", "rule_paths: path_off", "rule_paths: path_nodes",
         "rule_paths: path_facts", "rule_paths: workspace"]


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
    guarded.install(monkeypatch, guard)
    ops._rule_path_buffers.clear()              # cached (unguarded) buffers of earlier tests
    yield guard
    ops._rule_path_buffers.clear()
    guard.release()


def _inputs(dev, case, other_rules=False):
    rule_rel, rule_len = case["rule_rel"].copy(), case["rule_len"].copy()
    if other_rules:                             # the same shapes, other walks: what the leftovers run finds in its buffers
        rule_rel, rule_len = rule_rel[:, ::-1].copy(), rule_len[:, ::-1].copy()
    arrs = (case["rels"].astype(np.int32), case["seed_flag"].astype(np.uint8), rule_rel, rule_len)
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]


@pytest.mark.parametrize("name", ["tiny", "hub", "ragged"])
def test_rule_paths_in_guarded_buffers(dev, g, name):
    """The records behind path_off[P] are unspecified ("the rest of the two arrays is not touched"): the first
    path_off[-1] records are compared, everything else whole."""
    from gnnrag_amd import _lib, ops
    from test_gpu_rule_paths import _check_against_oracle, _host, _plan
    c = rule_paths_oracle.load_cases()[name]
    B, N = int(c["B"]), int(c["N"])
    graph = ops.UGraph.from_plan(_plan(c["heads"], c["rels"], c["tails"], B, N, int(c["R1"]), dev))
    S, R, K, H = 4, 8, 64, 4
    runs = []
    for fill, other in ((FILL_ZERO, False), (FILL_ZERO, True), (FILL_LEFTOVERS, False), (FILL_ONES, False)):
        g.fill = fill
        args = [g.wrap(t, "input %d" % i) for i, t in enumerate(_inputs(dev, c, other))]
        hits = g.leftover_hits
        buf = ops.RulePathBuffers(graph.F, B, N, S, R, K, H, dev)
        out = _host(ops.rule_paths(graph, *args, S, R, K, H, buffers=buf))
        if fill == FILL_LEFTOVERS:
            assert g.leftover_hits >= hits + len(ROLES)          # every output and the workspace held leftovers
        g.check("%s, body fill %r%s" % (name, fill, " (other rules)" if other else ""))
        if not other:
            runs.append(out)
    assert g.sizes["rule_paths: workspace"] == _lib.load().gnnrag_rule_paths_workspace_bytes(graph.F, B, N, R, H) > 256
    for role in ROLES:
        assert role in g.sizes
    for k in runs[0]:
        assert runs[0][k].tobytes() == runs[1][k].tobytes() == runs[2][k].tobytes(), (name, k)
    _check_against_oracle(runs[0], rule_paths_oracle.batch(c["heads"], c["rels"], c["tails"], B, N, c["seed_flag"],
                                                           c["rule_rel"], c["rule_len"], S, R, K, H), S, R, H)
    assert runs[0]["path_off"][-1] > 0


def test_workspace_one_byte_short_is_refused(dev, g):
    from gnnrag_amd import _lib, ops
    from test_gpu_rule_paths import _plan
    c = rule_paths_oracle.load_cases()["tiny"]
    B, N = int(c["B"]), int(c["N"])
    graph = ops.UGraph.from_plan(_plan(c["heads"], c["rels"], c["tails"], B, N, int(c["R1"]), dev))
    S, R, K, H = 4, 8, 64, 4
    args = _inputs(dev, c)
    role = "rule_paths: workspace"
    g.fill = FILL_ONES

    def call():
        buf = ops.RulePathBuffers(graph.F, B, N, S, R, K, H, dev)
        ops.rule_paths(graph, *args, S, R, K, H, buffers=buf)
        return buf

    call()                                                       # the stated size: accepted
    g.check("rule_paths at its stated size")
    g.short = {role: 1}                                          # the memory stays whole, only the stated size shrinks
    with pytest.raises(_lib.GnnragError, match=r"failed \(%d\)" % E_WORKSPACE):
        call()
    g.short = {}
    g.check("rule_paths one byte short")
    # nothing was launched: the outputs of the refused call still hold their body fill
    lib = _lib.load()
    buf = ops.RulePathBuffers(graph.F, B, N, S, R, K, H, dev)
    code = lib.gnnrag_rule_paths(C.byref(graph.c), *[a.data_ptr() for a in args], S, R, K, H, buf.q_info.data_ptr(),
                                 buf.pair_info.data_ptr(), buf.path_off.data_ptr(), buf.path_nodes.data_ptr(),
                                 buf.path_facts.data_ptr(), buf.ws.data_ptr(), buf.ws.numel() - 1,
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert code == E_WORKSPACE
    for x in (buf.q_info, buf.pair_info, buf.path_off, buf.path_nodes, buf.path_facts, buf.ws):
        assert (x.view(torch.uint8) == 0xFF).all()
    g.check("rule_paths refused")
