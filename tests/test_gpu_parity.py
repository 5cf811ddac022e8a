"""Parity of the HIP path (through the C ABI) against the CPU oracles and the golden
fixtures recorded from the live reference.  Run on the GPU box: pytest -m gpu.

Tolerances: the stated bar (BASELINE.json north_star) is 1e-4 fp32 on answer-node
scores; the tests assert that bar against the reference fixtures and a tighter
internal bound (2e-5) against the float64 oracle on the same inputs."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

TOL_STATED = 1e-4      # north_star: scores within 1e-4 fp32 of the reference CPU path
TOL_INTERNAL = 2e-5    # vs the float64 factored oracle


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()                      # the native library must be the thing under test
    return torch.device("cuda", 0)


def _csr_numpy(heads, rels, tails, B, N, R1):
    out = {}
    for d, (src, dst) in enumerate(((heads, tails), (tails, heads))):
        order = np.argsort(dst, kind="stable")
        # hub rows (more than 256 facts) are kept in relation order, stable inside a relation, when the vocabulary is
        # large enough for the gather walk to ever see them (csr_plan.hip: R1 > 1024)
        hub = (np.bincount(dst, minlength=B * N)[dst[order]] > 256) & (R1 > 1024)
        order = order[np.lexsort((np.where(hub, rels[order], 0), dst[order]))]
        out["perm%d" % d] = order.astype(np.int32)
        out["edge%d" % d] = np.stack([src[order], rels[order]], 1).astype(np.int32)
        out["row_ptr%d" % d] = np.searchsorted(dst[order], np.arange(B * N + 1), side="left").astype(np.int32)
    return out


@pytest.mark.parametrize("name", ["tiny", "mid", "tinyfb"])
def test_csr_plan_bit_exact(dev, name):
    from gnnrag_amd import ops, synth
    cfg = synth.CONFIGS[name] if name != "mid" else synth.GraphConfig(B=3, N=2000, E=10000, R=600, seed=5)
    batch = synth.make_batch(cfg)
    h, r, t = (np.asarray(batch.edge_tuple[i]) for i in range(3))
    plan = ops.CsrPlan(h, r, t, cfg.B, cfg.N, cfg.R1, dev)
    plan.attach_w_gnn(batch.edge_tuple[5])
    plan.attach_w_rel(batch.edge_tuple[6])
    got = plan.to_host()
    want = _csr_numpy(h, r, t, cfg.B, cfg.N, cfg.R1)
    for k, v in want.items():
        np.testing.assert_array_equal(got[k], v, err_msg=k)
    wl = np.asarray(batch.edge_tuple[5], np.float32)
    wrl = np.asarray(batch.edge_tuple[6], np.float32)
    for d in (0, 1):
        np.testing.assert_array_equal(got["w_gnn"][d], (wl * wl)[want["perm%d" % d]])
        np.testing.assert_array_equal(got["w_rel"][d], wrl[want["perm%d" % d]])
        deg = np.diff(want["row_ptr%d" % d])
        hubs = np.flatnonzero(deg > 256)
        np.testing.assert_array_equal(got["heavy%d" % d], hubs.astype(np.int32))     # ascending: question by question
        per_q = np.bincount(hubs // cfg.N, minlength=cfg.B)
        np.testing.assert_array_equal(got["hub_q_off%d" % d], np.concatenate([[0], np.cumsum(per_q)]))
        assert got["n_chunks"][d] == int(np.ceil(deg[deg > 256] / 256).sum())
    deg2 = np.maximum(np.diff(want["row_ptr0"]), np.diff(want["row_ptr1"])).reshape(cfg.B, cfg.N)
    for b in range(cfg.B):
        np.testing.assert_array_equal(got["big"][b], b * cfg.N + np.flatnonzero(deg2[b] > 32))
    # per-question relation compaction: rows = sorted distinct (question, relation) pairs
    pairs = np.unique(np.stack([h // cfg.N, r], 1), axis=0)
    np.testing.assert_array_equal(got["rel_rows"], pairs)
    cnt = np.bincount(pairs[:, 0], minlength=cfg.B) if len(pairs) else np.zeros(cfg.B, np.int64)
    np.testing.assert_array_equal(got["rel_off"], np.concatenate([[0], np.cumsum(cnt)]))
    assert plan.rel_total == len(pairs) and plan.rel_max == int(cnt.max())
    for d in (0, 1):        # offsets of the per-question hub-by-relation weight blocks (dense hub form of the gather walk)
        per_q = np.diff(got["hub_q_off%d" % d])
        np.testing.assert_array_equal(got["hub_wbase%d" % d], np.concatenate([[0], np.cumsum(per_q * ((cnt + 3) // 4 * 4))]))
    for d in (0, 1):
        e, el = got["edge%d" % d], got["edge_l%d" % d]
        np.testing.assert_array_equal(el[:, 0], e[:, 0])
        q = e[:, 0] // cfg.N
        np.testing.assert_array_equal(got["rel_rows"][got["rel_off"][q] + el[:, 1]], np.stack([q, e[:, 1]], 1))
    # merged rows: node n's facts of direction 0, then of direction 1, as one run of a 2F-long record stream; direction
    # 1's compact relation index is moved behind direction 0's table slice (+ relations of the question + 1)
    dst = {0: t, 1: h}
    rp0, rp1 = want["row_ptr0"].astype(np.int64), want["row_ptr1"].astype(np.int64)
    F = len(h)
    nrel = np.diff(got["rel_off"])
    em = np.zeros((2 * F, 2), np.int64)
    frm = np.zeros(2 * F, np.int64)
    mdst = np.zeros(2 * F, np.int64)
    for d in (0, 1):
        n_of = dst[d][want["perm%d" % d]]                          # destination of every sorted position
        m = np.arange(F) + (rp1[n_of] if d == 0 else rp0[n_of + 1])
        rec = got["edge_l%d" % d].astype(np.int64).copy()
        if d == 1:
            rec[:, 1] += nrel[n_of // cfg.N] + 1
        em[m] = rec
        frm[m] = d * F + np.arange(F)
        mdst[m] = n_of
    np.testing.assert_array_equal(got["m_dst"], mdst)              # destination node of every merged record
    np.testing.assert_array_equal(got["edge_m"], em)
    np.testing.assert_array_equal(got["m_from"], frm)
    assert np.array_equal(np.sort(frm), np.arange(2 * F))           # every fact of both directions exactly once
    if name == "mid":
        assert got["n_heavy"].sum() > 0, "the Zipf hub must exercise the heavy-row path"


@pytest.mark.parametrize("form", ["keys", "segmented"])
def test_csr_hub_rows_in_relation_order(dev, form, monkeypatch):
    """Hub rows (> 256 facts) of a large vocabulary are stored in (relation, fact id) order (csr_plan.hip: one stable sort
    over (segment, relation) keys; GNNRAG_HUB_SORT=segmented = rocPRIM's segmented sort, the form for keys wider than 32
    bits): both forms against numpy's lexsort, on hubs placed where a segment search can go wrong - the first row, two
    adjacent rows, the last row of a question, the last row of the batch, a question without any, in both directions."""
    from gnnrag_amd import ops
    if form == "segmented":
        monkeypatch.setenv("GNNRAG_HUB_SORT", "segmented")
    else:
        monkeypatch.delenv("GNNRAG_HUB_SORT", raising=False)
    rng = np.random.default_rng(11)
    B, N, R1 = 4, 300, 3000
    parts = []

    def star(q, hub, n, inverse):              # n facts between random nodes of question q and its node `hub`
        other = q * N + rng.integers(0, N, n)
        centre = np.full(n, q * N + hub)
        rel = rng.integers(0, R1, n)
        parts.append((centre, rel, other) if inverse else (other, rel, centre))

    star(0, 0, 700, False); star(0, 1, 300, False); star(0, 1, 280, True)
    star(1, N - 1, 500, False); star(1, 150, 257, True); star(1, 151, 256, True)      # 256 facts: NOT a hub
    star(3, N - 1, 900, True); star(3, N - 2, 400, True); star(3, N - 1, 300, False)
    for q in range(B):                         # ordinary rows around them (question 2 has nothing else)
        n = 1500
        parts.append((q * N + rng.integers(0, N, n), rng.integers(0, R1, n), q * N + rng.integers(0, N, n)))
    h = np.concatenate([p[0] for p in parts]).astype(np.int32)
    r = np.concatenate([p[1] for p in parts]).astype(np.int32)
    t = np.concatenate([p[2] for p in parts]).astype(np.int32)
    mix = rng.permutation(len(h))
    h, r, t = h[mix], r[mix], t[mix]
    got = ops.CsrPlan(h, r, t, B, N, R1, dev).to_host()
    want = _csr_numpy(h, r, t, B, N, R1)
    for k, v in want.items():
        np.testing.assert_array_equal(got[k], v, err_msg="%s (%s)" % (k, form))
    for d in (0, 1):
        deg = np.diff(want["row_ptr%d" % d])
        assert (deg > 256).sum() >= 4 and (deg == 0).any()
        np.testing.assert_array_equal(got["heavy%d" % d], np.flatnonzero(deg > 256).astype(np.int32))


def test_csr_plan_empty_and_validation(dev):
    from gnnrag_amd import ops
    z = np.zeros(0, np.int64)
    plan = ops.CsrPlan(z, z, z, 2, 8, 3, dev)
    got = plan.to_host()
    assert (got["row_ptr0"] == 0).all() and (got["row_ptr1"] == 0).all()
    assert plan.rel_total == 0 and plan.rel_max == 0 and (got["rel_off"] == 0).all()
    with pytest.raises(ValueError):
        ops.CsrPlan(np.array([0]), np.array([5]), np.array([1]), 1, 8, 3, dev)      # relation out of range
    with pytest.raises(ValueError):
        ops.CsrPlan(np.array([0]), np.array([0]), np.array([9]), 2, 8, 3, dev)      # crosses questions
    with pytest.raises(ValueError):
        ops.CsrPlan(np.array([0, 16]), np.array([0, 1]), np.array([1, 16]), 2, 8, 3, dev)   # node id >= B*N
    with pytest.raises(ValueError):
        ops.CsrPlan(np.array([-1]), np.array([0]), np.array([-1]), 2, 8, 3, dev)    # negative node id
    plan = ops.CsrPlan(np.array([0, 9]), np.array([2, 0]), np.array([7, 15]), 2, 8, 3, dev)   # valid again afterwards
    assert plan.rel_total == 2


@pytest.mark.parametrize("M,K,Nout,with_add,relu", [
    (602, 200, 200, False, False), (602, 200, 200, True, False), (9, 50, 50, True, True),
    (300, 250, 50, False, True), (130, 64, 300, False, False), (1, 8, 8, False, False),
    (257, 1000, 200, False, True)])
def test_linear_vs_fp64(dev, M, K, Nout, with_add, relu):
    """gnnrag_linear on k_gemm_skinny (every shape here has M <= 16384) against float64; the k-tiled kernel is held to
    float64 form by form in tests/test_gpu_dense_forms.py."""
    from gnnrag_amd import ops
    assert ops.dense_form("linear", M, K, Nout, add_rows=max(M - 1, 1) if with_add else None).family == ops.DENSE_SKINNY
    rng = np.random.default_rng(M + K)
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((Nout, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(Nout).astype(np.float32)
    add = rng.standard_normal((max(M - 1, 1), Nout)).astype(np.float32) if with_add else None
    want = A.astype(np.float64) @ W.astype(np.float64).T + b
    if with_add:
        want[: add.shape[0]] += add
    if relu:
        want = np.maximum(want, 0)
    got = ops.linear(torch.from_numpy(A).to(dev), torch.from_numpy(W).to(dev), torch.from_numpy(b).to(dev),
                     None if add is None else torch.from_numpy(add).to(dev), relu=relu).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=0, atol=5e-6 * np.sqrt(K))


@pytest.mark.parametrize("R1,D,L,pos_rows", [(602, 200, 3, 0), (602, 200, 3, 602), (12, 56, 2, 7), (1, 8, 1, 0),
                                             (6106, 200, 4, 0), (130, 36, 9, 130), (3001, 208, 2, 2500)])
def test_rel_transform_all_layers_in_one_launch_vs_fp64(dev, R1, D, L, pos_rows):
    """gnnrag_rel_transform (k_rel_transform): rel_linear{j}(rel_features_d) (+ pos_emb{j}_d) for every layer j and
    both directions from one launch (L = 9 takes two launches), against fp64; reasongnn.py:75-79, :102-105."""
    from gnnrag_amd import ops
    rng = np.random.default_rng(R1 + D + L)
    A = [rng.standard_normal((R1, D)).astype(np.float32) for _ in range(2)]
    layers, want = [], np.zeros((L, 2, R1, D))
    for j in range(L):
        W = (rng.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32)
        b = rng.standard_normal(D).astype(np.float32)
        pos = [rng.standard_normal((pos_rows, D)).astype(np.float32) for _ in range(2)] if pos_rows else [None, None]
        for d in range(2):
            want[j, d] = A[d].astype(np.float64) @ W.astype(np.float64).T + b
            if pos_rows:
                want[j, d, :pos_rows] += pos[d]
        layers.append(tuple(None if x is None else torch.from_numpy(x).to(dev) for x in (W, b, pos[0], pos[1])))
    got = ops.rel_transform(torch.from_numpy(A[0]).to(dev), torch.from_numpy(A[1]).to(dev), layers).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=0, atol=5e-6 * np.sqrt(D))
    # the skinny k-tiled kernel the projections ran on before (same exact-fp32 matrix-core arithmetic class)
    old = ops.linear(torch.from_numpy(A[1]).to(dev), layers[-1][0], layers[-1][1], layers[-1][3],
                     math=ops.MATH_FP32).cpu().numpy()
    np.testing.assert_allclose(got[-1, 1], old, rtol=0, atol=2e-6 * np.sqrt(D))


def _to_dev(dev, *arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]


@pytest.mark.parametrize("cfgname", ["tiny", "tiny50", "hub"])
def test_aggregate_and_update_vs_np64(dev, cfgname):
    """Each kernel on its own against the float64 factored oracle (first layer call and a
    dense-prior call), incl. the heavy-row path (cfg 'hub')."""
    import oracle.rearev_np64 as onp
    from gnnrag_amd import ops, synth
    if cfgname == "hub":
        cfg = synth.GraphConfig(name="hub", B=2, N=600, E=4000, R=20, D=200, I=2, L=1, seed=3)
    else:
        cfg = synth.CONFIGS[cfgname]
    batch = synth.make_batch(cfg)
    feats = synth.make_features(cfg)
    params = synth.make_layer_params(cfg)
    B, N, D, I = cfg.B, cfg.N, cfg.D, cfg.I
    mask = (batch.local_entity != batch.num_entity).astype(np.float32)
    rng = np.random.default_rng(0)
    dense = rng.random((B, N)).astype(np.float32)
    dense /= dense.sum(1, keepdims=True)
    et = batch.edge_tuple
    plan = ops.CsrPlan(et[0], et[1], et[2], B, N, cfg.R1, dev)
    if cfg.normalized_gnn:
        plan.attach_w_gnn(et[5])
    for prior in (batch.seed_dist.astype(np.float32), dense):
        score, nd, hn, agg = onp.layer_call(et, B, N, feats["h0"], mask, prior, feats["ins"][0], params, 0,
                                            feats["rel_features"], feats["rel_features_inv"],
                                            normalized_gnn=cfg.normalized_gnn, use_posemb=cfg.pos_emb)
        W_r, b_r = params["rel_linear0.weight"], params["rel_linear0.bias"]
        rf, rfi, Wd, bd = _to_dev(dev, feats["rel_features"], feats["rel_features_inv"], W_r, b_r)
        pos = posi = None
        if cfg.pos_emb:
            pos, posi = _to_dev(dev, params["pos_emb0.weight"], params["pos_emb_inv0.weight"])
        T_f = ops.linear(rf, Wd, bd, pos)
        T_i = ops.linear(rfi, Wd, bd, posi)
        dist_d, ins_d = _to_dev(dev, prior, feats["ins"][0])
        got_agg = ops.aggregate(plan, dist_d, ins_d, T_f, T_i).cpu().numpy().reshape(B * N, 2 * I, D)
        scale = max(1.0, float(np.abs(agg).max()))
        np.testing.assert_allclose(got_agg, agg, rtol=0, atol=TOL_INTERNAL * scale)
        # update + score on the oracle's own agg (isolates the GEMM epilogue)
        h_d, agg_d, We, be, ws, bs, mk = _to_dev(
            dev, feats["h0"].reshape(B * N, D), agg.reshape(B * N, -1).astype(np.float32),
            params["e2e_linear0.weight"], params["e2e_linear0.bias"], params["score_func.weight"],
            params["score_func.bias"], mask)
        h_out, sc = ops.update_score(h_d, agg_d, We, be, ws, bs, mk, I)
        np.testing.assert_allclose(h_out.cpu().numpy(), hn.reshape(B * N, D), rtol=0, atol=TOL_INTERNAL)
        valid = mask.reshape(-1) > 0
        np.testing.assert_allclose(sc.cpu().numpy()[valid], score.reshape(-1)[valid], rtol=0, atol=TOL_INTERNAL)
        assert (sc.cpu().numpy()[~valid] == np.float32(-1e11)).all()
        got_dist = ops.masked_softmax(sc, B, N).cpu().numpy()
        np.testing.assert_allclose(got_dist, nd, rtol=0, atol=1e-6)


@pytest.mark.parametrize("path", [1, 2], ids=["unfused", "fused"])
@pytest.mark.parametrize("name", ["layer_d200.npz", "layer_d50.npz"])
def test_layer_stack_matches_reference_fixture(dev, name, path):
    from gnnrag_amd import stack
    cfg, batch, feats, params, ref = load_golden(name)
    out = stack.run_stack(batch, feats, params, dev, path=path)
    mask = batch.local_entity != batch.num_entity
    for c in range(cfg.T * cfg.L):
        dh = np.abs(out["h"][c] - ref["h"][c]).max()
        dd = np.abs(out["dist"][c] - ref["dist"][c]).max()
        ds = np.abs(out["score"][c][mask] - ref["score"][c][mask]).max() if mask.any() else 0.0
        assert dh <= TOL_STATED and dd <= TOL_STATED and ds <= TOL_STATED, (c, dh, dd, ds)
        assert dh <= TOL_INTERNAL and ds <= TOL_INTERNAL, (c, dh, ds)      # tighter internal bound
        assert (out["dist"][c].argmax(1) == ref["dist"][c].argmax(1)).all()
        np.testing.assert_array_equal(out["score"][c][~mask], ref["score"][c][~mask])   # exactly -1e11
    # all-masked question: exactly uniform, like the reference
    some = mask.any(axis=1)
    if (~some).any():
        np.testing.assert_array_equal(out["dist"][-1][~some], ref["dist"][-1][~some])


@pytest.mark.parametrize("case", ["c2_like", "weights_d50", "wide_rows"])
def test_softmax_with_next_layers_pairs_is_bit_identical(dev, case, monkeypatch):
    """Inside the whole-iteration call a layer's last launch writes the distribution AND the next layer's (prior,
    relation) pairs (k_softmax_pairs; softmax_layer.hip) instead of leaving the pairs to a pass of the walk
    (k_fact_prior_merged): same arithmetic, so every tensor of the stack is bit-identical to the two-launch form
    (GNNRAG_SOFTMAX_PAIRS=0) - without and with per-fact weights (reasongnn.py:106-111 under normalized_gnn), and with more
    than 2048 node slots per question (the 8-scores-per-thread softmax)."""
    from gnnrag_amd import stack, synth
    cfg = {"c2_like": synth.GraphConfig(name="c2_like", B=5, N=2000, E=10000, R=600, D=200, I=2, L=3, T=2, seed=3),
           "weights_d50": synth.GraphConfig(name="w50", B=4, N=700, E=3000, R=40, D=50, I=3, L=3, T=2, normalized_gnn=True,
                                            pos_emb=True, seed=4),
           "wide_rows": synth.GraphConfig(name="wide", B=2, N=3000, E=9000, R=300, D=200, I=2, L=2, T=1, seed=5)}[case]
    batch = synth.make_batch(cfg)
    feats = synth.make_features(cfg)
    params = synth.make_layer_params(cfg)
    monkeypatch.setenv("GNNRAG_SOFTMAX_PAIRS", "0")
    two = stack.run_stack(batch, feats, params, dev, path=2)
    monkeypatch.delenv("GNNRAG_SOFTMAX_PAIRS")
    one = stack.run_stack(batch, feats, params, dev, path=2)
    for key in ("h", "score", "dist"):
        for c in range(cfg.T * cfg.L):
            np.testing.assert_array_equal(one[key][c], two[key][c], err_msg="%s[%d]" % (key, c))
    assert np.isfinite(one["dist"][-1]).all() and abs(one["dist"][-1].sum(1) - 1).max() < 1e-4


@pytest.mark.parametrize("norm_rel", [False, True])
def test_type_layer_matches_reference_fixture(dev, norm_rel):
    from gnnrag_amd import stack, synth
    z = np.load(os.path.join(GOLDEN, "typelayer.npz"))
    B, N, D = int(z["B"]), int(z["N"]), int(z["D"])
    F = len(z["heads"])
    et = (z["heads"], z["rels"], z["tails"], z["batch_ids"], np.arange(F), z["weight_list"].tolist(),
          z["weight_rel_list"].tolist())
    cfg = synth.GraphConfig(B=B, N=N, D=D, R=int(z["R1"]) - 2)
    params = {"type_layer.kb_self_linear.weight": z["param.type_layer.kb_self_linear.weight"],
              "type_layer.kb_self_linear.bias": z["param.type_layer.kb_self_linear.bias"]}
    tl = stack.build_type_layer(cfg, params, dev, norm_rel)
    with torch.no_grad():
        h0 = tl(local_entity=torch.from_numpy(z["local_entity"]).to(dev), edge_list=et,
                rel_features=torch.from_numpy(z["feat.rel_features"]).to(dev)).cpu().numpy()
    np.testing.assert_allclose(h0, z["ref.h0_norm%d" % int(norm_rel)], rtol=0, atol=TOL_INTERNAL)


def test_rearev_call_site_fixture(dev):
    """Tensors recorded at the layer boundary inside a real ReaRev.forward (dataset_load ->
    get_batch -> model): feeding the recorded inputs through the drop-in module reproduces the
    recorded outputs and the model's final prediction."""
    from gnnrag_amd.modules.kg_reasoning.reasongnn import ReasonGNNLayer
    z = np.load(os.path.join(GOLDEN, "rearev_e2e.npz"))
    B, N, D, I, L = (int(z[k]) for k in ("B", "N", "D", "I", "L"))
    F = len(z["heads"])
    et = (z["heads"], z["rels"], z["tails"], z["batch_ids"], np.arange(F), z["weight_list"].tolist(),
          z["weight_rel_list"].tolist())
    args = dict(use_cuda=True, normalized_gnn=False, num_ins=I, num_gnn=L, pos_emb=False, linear_dropout=0.0)
    layer = ReasonGNNLayer(args, int(z["num_entity"]), int(z["num_kb_relation"]), D, "bfs")
    layer.load_state_dict({k[6:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param.")}, strict=True)
    layer.to(dev).eval()
    with torch.no_grad():
        layer.init_reason(local_entity=torch.from_numpy(z["local_entity"]).to(dev), kb_adj_mat=et,
                          local_entity_emb=torch.from_numpy(z["h0"]).to(dev),
                          rel_features=torch.from_numpy(z["rel_features"]).to(dev),
                          rel_features_inv=torch.from_numpy(z["rel_features_inv"]).to(dev),
                          query_entities=torch.from_numpy(z["query_entities"]).to(dev))
        for c, step in enumerate(z["call.step"]):
            dist, h = layer(torch.from_numpy(z["call.dist_in"][c]).to(dev),
                            torch.from_numpy(z["call.ins"][c]).to(dev), step=int(step))
            assert np.abs(dist.cpu().numpy() - z["call.dist_out"][c]).max() <= TOL_INTERNAL
            assert np.abs(h.cpu().numpy() - z["call.h_out"][c]).max() <= TOL_INTERNAL
    assert np.abs(dist.cpu().numpy() - z["pred_dist"]).max() <= TOL_STATED
    assert (dist.cpu().numpy().argmax(1) == z["pred"]).all()          # Hits@1 decisions identical


@pytest.mark.parametrize("cfgname", ["tiny", "tiny50", "hub", "huge", "tinyfb"])
def test_fused_kernels_vs_np64(dev, cfgname):
    """The fused path's own kernels (relation tables, fused walk incl. heavy chunks and the
    XCD-aware order, self-block update) against the float64 oracle."""
    import oracle.rearev_np64 as onp
    from gnnrag_amd import ops, synth
    if cfgname == "hub":      # rows of 33..4096 facts: the wave-per-node class of the LDS walk
        cfg = synth.GraphConfig(name="hub", B=3, N=600, E=4000, R=20, D=200, I=2, L=1, seed=3)
    elif cfgname == "huge":   # a row with > 4096 facts: the workgroup-per-node class
        cfg = synth.GraphConfig(name="huge", B=2, N=500, E=14000, R=20, D=200, I=2, L=1, seed=4)
    else:
        cfg = synth.CONFIGS[cfgname]
    batch = synth.make_batch(cfg)
    feats = synth.make_features(cfg)
    params = synth.make_layer_params(cfg)
    B, N, D, I = cfg.B, cfg.N, cfg.D, cfg.I
    mask = (batch.local_entity != batch.num_entity).astype(np.float32)
    rng = np.random.default_rng(0)
    dense = rng.random((B, N)).astype(np.float32)
    dense /= dense.sum(1, keepdims=True)
    et = batch.edge_tuple
    plan = ops.CsrPlan(et[0], et[1], et[2], B, N, cfg.R1, dev)
    if cfg.normalized_gnn:
        plan.attach_w_gnn(et[5])
    W_e = params["e2e_linear0.weight"].astype(np.float64)
    for prior in (batch.seed_dist.astype(np.float32), dense):
        score, nd, hn, agg = onp.layer_call(et, B, N, feats["h0"], mask, prior, feats["ins"][0], params, 0,
                                            feats["rel_features"], feats["rel_features_inv"],
                                            normalized_gnn=cfg.normalized_gnn, use_posemb=cfg.pos_emb)
        want_nbr = agg.reshape(B * N, 2 * I * D) @ W_e[:, D:].T
        rf, rfi, Wd, bd = _to_dev(dev, feats["rel_features"], feats["rel_features_inv"],
                                  params["rel_linear0.weight"], params["rel_linear0.bias"])
        pos = posi = None
        if cfg.pos_emb:
            pos, posi = _to_dev(dev, params["pos_emb0.weight"], params["pos_emb_inv0.weight"])
        T_f = ops.linear(rf, Wd, bd, pos)
        T_i = ops.linear(rfi, Wd, bd, posi)
        dist_d, ins_d, We = _to_dev(dev, prior, feats["ins"][0], params["e2e_linear0.weight"])
        if cfgname == "huge":
            deg = np.bincount(np.asarray(et[0]), minlength=B * N)
            assert deg.max() > 4096, "config must exercise the workgroup-per-node class"
        P = ops.relation_tables(plan, T_f, T_i, ins_d, We)
        # tables vs fp64
        Tn = [feats["rel_features"].astype(np.float64) @ params["rel_linear0.weight"].astype(np.float64).T
              + params["rel_linear0.bias"], feats["rel_features_inv"].astype(np.float64)
              @ params["rel_linear0.weight"].astype(np.float64).T + params["rel_linear0.bias"]]
        if cfg.pos_emb:
            Tn[0][: cfg.num_kb_relation] += params["pos_emb0.weight"]
            Tn[1][: cfg.num_kb_relation] += params["pos_emb_inv0.weight"]
        Pw = np.zeros((2, B, cfg.R1, D))
        for d in range(2):
            for i in range(I):
                blk = W_e[:, (1 + 2 * i + d) * D:(2 + 2 * i + d) * D]
                Pw[d] += np.maximum(Tn[d][None] * feats["ins"][0][:, i, None, :].astype(np.float64), 0) @ blk.T
        rows = plan.rel_rows()          # compact rows: (question, relation the question uses)
        used = {(int(h) // N, int(r)) for h, r in zip(et[0], et[1])}
        assert [tuple(x) for x in rows.tolist()] == sorted(used)
        Pw = Pw[:, rows[:, 0], rows[:, 1], :]
        np.testing.assert_allclose(P.cpu().numpy(), Pw, rtol=0, atol=TOL_INTERNAL * max(1.0, np.abs(Pw).max()))
        nbr = ops.aggregate_fused(plan, dist_d, P)
        np.testing.assert_allclose(nbr.cpu().numpy(), want_nbr, rtol=0,
                                   atol=TOL_INTERNAL * max(1.0, np.abs(want_nbr).max()))
        h_d, be, ws, bs, mk = _to_dev(dev, feats["h0"].reshape(B * N, D), params["e2e_linear0.bias"],
                                      params["score_func.weight"], params["score_func.bias"], mask)
        h_out, sc = ops.update_score_fused(h_d, nbr, We, be, ws, bs, mk, I)
        np.testing.assert_allclose(h_out.cpu().numpy(), hn.reshape(B * N, D), rtol=0, atol=TOL_INTERNAL)
        valid = mask.reshape(-1) > 0
        np.testing.assert_allclose(sc.cpu().numpy()[valid], score.reshape(-1)[valid], rtol=0, atol=TOL_INTERNAL)


@pytest.mark.parametrize("path", [1, 2], ids=["unfused", "fused"])
def test_mid_size_vs_torch_cpu_oracle(dev, path):
    """C2-shaped questions (N=2000, E=10000 Zipf, hubs > 256 in-degree) at a batch the CPU
    restatement finishes in seconds."""
    import oracle.rearev_torch_cpu as otorch
    from gnnrag_amd import stack, synth
    cfg = synth.GraphConfig(name="mid", B=4, N=2000, E=10000, R=600, D=200, I=2, L=3, T=2, seed=21)
    batch = synth.make_batch(cfg)
    feats = synth.make_features(cfg)
    params = synth.make_layer_params(cfg)
    want = otorch.run_stack(batch, feats, params)
    got = stack.run_stack(batch, feats, params, dev, path=path)
    for c in range(cfg.T * cfg.L):
        assert np.abs(got["h"][c] - want["h"][c]).max() <= TOL_STATED, c
        assert np.abs(got["dist"][c] - want["dist"][c]).max() <= TOL_STATED, c
        assert (got["dist"][c].argmax(1) == want["dist"][c].argmax(1)).all()


@pytest.mark.parametrize("path", [1, 2], ids=["unfused", "fused"])
def test_full_size_properties_c2(dev, path):
    """BASELINE config C2 at full size through size-independent properties: probabilities sum
    to 1 and vanish on masked slots; the aggregation is linear in the prior; two runs are
    bit-identical; a batch split into two shards reproduces the whole batch bit for bit."""
    from gnnrag_amd import ops, shard, stack, synth
    cfg = synth.CONFIGS["C2"]
    batch = synth.make_batch(cfg)
    feats = synth.make_features(cfg)
    params = synth.make_layer_params(cfg)
    devin = stack.DeviceInputs(batch, feats, dev)
    layer = stack.build_layer(cfg, batch, params, dev, path)
    stack.init_reason(layer, batch, devin, devin.h0)
    dist, _ = stack.run_layers(layer, cfg, devin)
    h_full = layer.local_entity_emb.clone()
    d = dist.cpu().numpy()
    mask = batch.local_entity != batch.num_entity
    np.testing.assert_allclose(d.sum(1), 1.0, atol=1e-5)
    assert (d[~mask] == 0).all() and np.isfinite(d).all()
    # determinism
    stack.init_reason(layer, batch, devin, devin.h0)
    dist2, _ = stack.run_layers(layer, cfg, devin)
    assert torch.equal(dist, dist2) and torch.equal(h_full, layer.local_entity_emb)
    # linearity of the aggregation in the prior
    plan = layer.plan
    rng = np.random.default_rng(1)
    p1 = torch.from_numpy(rng.random((cfg.B, cfg.N)).astype(np.float32)).to(dev)
    p2 = torch.from_numpy(rng.random((cfg.B, cfg.N)).astype(np.float32)).to(dev)
    T = ops.linear(devin.rel_features, layer.rel_linear0.weight, layer.rel_linear0.bias)
    ins = devin.ins[0]
    a1 = ops.aggregate(plan, p1, ins, T, T)
    a2 = ops.aggregate(plan, p2, ins, T, T)
    a12 = ops.aggregate(plan, p1 + p2, ins, T, T)
    err = (a12 - (a1 + a2)).abs().max().item()
    assert err <= 1e-4 * max(1.0, a12.abs().max().item()), err
    # sharding invariance (the multi-GPU layout on one device): bit-identical
    ref_batch = (batch.local_entity, batch.query_entities, batch.edge_tuple, np.zeros((cfg.B, 1)),
                 batch.seed_dist, None, np.zeros((cfg.B, cfg.N)))
    parts = []
    for r in range(2):
        lo, hi = shard.question_range(cfg.B, r, 2)
        sb = shard.shard_batch(ref_batch, r, 2)
        sub = synth.Batch(cfg=synth.GraphConfig(**{**cfg.__dict__, "B": hi - lo}), local_entity=sb[0],
                          query_entities=sb[1], seed_dist=sb[4], edge_tuple=sb[2],
                          num_entity=batch.num_entity, n_real=batch.n_real[lo:hi])
        sfe = dict(feats)
        sfe["h0"] = feats["h0"][lo:hi]
        sfe["ins"] = feats["ins"][:, lo:hi]
        sdev = stack.DeviceInputs(sub, sfe, dev)
        slayer = stack.build_layer(sub.cfg, sub, params, dev, path)
        stack.init_reason(slayer, sub, sdev, sdev.h0)
        sd, _ = stack.run_layers(slayer, sub.cfg, sdev)
        parts.append(sd)
    assert torch.equal(torch.cat(parts, 0), dist)


def test_freebase_vocabulary_picks_fused_path(dev):
    """WebQSP-sized relation vocabulary (6105 ids), a few hundred used per question: the tables are built
    over the used relations only, so the fused path stays cheaper (and fits LDS); both paths agree with the
    torch-CPU restatement."""
    import oracle.rearev_torch_cpu as otorch
    from gnnrag_amd import ops, stack, synth
    cfg = synth.GraphConfig(name="fb", B=4, N=2000, E=10000, R=6105, D=200, I=2, L=3, T=1, seed=33,
                            rel_per_question=300)
    batch = synth.make_batch(cfg)
    feats = synth.make_features(cfg)
    params = synth.make_layer_params(cfg)
    et = batch.edge_tuple
    plan = ops.CsrPlan(et[0], et[1], et[2], cfg.B, cfg.N, cfg.R1, dev)
    assert plan.rel_max <= 301 and plan.rel_total <= cfg.B * 301      # 300 drawn + the self-loop relation
    want = otorch.run_stack(batch, feats, params)
    for path in (0, 1, 2):
        got = stack.run_stack(batch, feats, params, dev, path=path)
        for c in range(cfg.T * cfg.L):
            assert np.abs(got["h"][c] - want["h"][c]).max() <= TOL_STATED, (path, c)
            assert np.abs(got["dist"][c] - want["dist"][c]).max() <= TOL_STATED, (path, c)
            assert (got["dist"][c].argmax(1) == want["dist"][c].argmax(1)).all()


@pytest.mark.parametrize("B,N,E,R,D,I", [
    (1, 17, 40, 3, 64, 1),        # one question, N not a multiple of 16, 16-lane walk groups, NT=4 GEMM
    (2, 50, 200, 9, 100, 4),      # I > 3: two instruction passes; D=100 -> 32-lane groups, NT=8 GEMM
    (2, 33, 150, 5, 128, 2),
    (3, 70, 300, 6, 256, 3),      # D > 208: column-blocked update + separate score kernel
    (2, 40, 160, 4, 300, 2),      # two float4 chunks per lane
    (2, 30, 100, 5, 36, 2),       # D % 4 == 0 but tiny
    (2, 30, 100, 5, 30, 2),       # D % 4 != 0: float2 walk, scalar GEMM loaders
    (2, 30, 100, 5, 25, 1),       # odd D: scalar everything
    (5, 1800, 9000, 400, 208, 2),  # D = 208, >= 8192 rows, >= 1024 compact rows: the bf16x3 W-resident kernels at their
                                   # other admissible hidden size (k_tables_vq, k_update_b3; 13 full column tiles)
    (5, 1800, 9000, 400, 200, 3),  # ... and with three instructions (V form: k extent 2D regardless)
])
def test_shape_sweep_both_paths_vs_np64(dev, B, N, E, R, D, I):
    """Odd shapes through every dispatch branch (vector width, lane-group size, GEMM tile variants,
    instruction passes), both kernel paths, against the float64 oracle."""
    import oracle.rearev_np64 as onp
    from gnnrag_amd import stack, synth
    cfg = synth.GraphConfig(name="sweep", B=B, N=N, E=E, R=R, D=D, I=I, L=2, T=2, seed=B * 1000 + D,
                            normalized_gnn=(D % 2 == 0), pos_emb=(I % 2 == 1), n_real_min=max(2, N // 2))
    batch = synth.make_batch(cfg)
    feats = synth.make_features(cfg)
    params = synth.make_layer_params(cfg)
    want = onp.run_stack(batch, feats, params, use_type_layer=True, norm_rel=True)
    for path in (1, 2):
        got = stack.run_stack(batch, feats, params, dev, use_type_layer=True, norm_rel=True, path=path)
        # node embeddings: fp32 rounding scales with their magnitude (a TypeLayer start sums hundreds of facts at the
        # hubs of the larger cases); distributions are <= 1
        np.testing.assert_allclose(got["h0"], want["h0"], rtol=0, atol=TOL_INTERNAL * max(1.0, np.abs(want["h0"]).max()),
                                   err_msg="h0 path %d" % path)
        for c in range(cfg.T * cfg.L):
            np.testing.assert_allclose(got["h"][c], want["h"][c], rtol=0,
                                       atol=TOL_INTERNAL * max(1.0, np.abs(want["h"][c]).max()),
                                       err_msg="h call %d path %d" % (c, path))
            np.testing.assert_allclose(got["dist"][c], want["dist"][c], rtol=0, atol=TOL_INTERNAL,
                                       err_msg="dist call %d path %d" % (c, path))


# The binding's default math mode is MATH_MIXED (per kernel the faster fp32-class form), so every test above runs
# that mode; the tests below repeat the reference-fixture and oracle gates with the mode pinned to bf16x3 (param
# "bf16x3") and to exact fp32 ("fp32") everywhere.
@pytest.fixture(params=["bf16x3", "fp32"])
def bf16x3(dev, request):
    from gnnrag_amd import ops
    old = ops.set_dense_math(ops.MATH_BF16X3 if request.param == "bf16x3" else ops.MATH_FP32)
    yield request.param
    ops.set_dense_math(old)


@pytest.mark.parametrize("M,K,Nout", [(5000, 200, 200), (6000, 1000, 200), (4500, 250, 50), (40000, 400, 200),
                                      (16391, 1000, 200), (20000, 250, 50), (16391, 200, 1000)])
def test_bf16x3_linear_is_fp32_class(dev, bf16x3, M, K, Nout):
    """The split-bf16 math mode against float64, and against the exact-fp32 MFMA mode: its error must
    be of the same class (fp32 rounding), not bf16 class.  Up to 16384 rows both modes run k_gemm_skinny (exact fp32:
    the comparison is then of a kernel with itself, kept as the proof that the skinny kernel ignores the mode); the
    shapes above run k_gemm_f32 - its two MFMA forms where K % 4 == 0, (16391, 200, 1000) through five column blocks."""
    from gnnrag_amd import ops
    f3 = ops.dense_form("linear", M, K, Nout, math=ops.MATH_BF16X3)
    f32 = ops.dense_form("linear", M, K, Nout, math=ops.MATH_FP32)
    if M <= 16384:
        assert f3 == f32 and f3.family == ops.DENSE_SKINNY
    else:
        # K % 4 != 0 takes the scalar loaders, which exist in the exact-fp32 form only: (20000, 250, 50) runs the SAME
        # k_gemm_f32 instantiation in both modes, the other two shapes its two MFMA forms
        assert f3.family == f32.family == ops.DENSE_KTILED and (f3.math, f32.math) == (int(K % 4 == 0), 0)
        assert f3._replace(math=0) == f32 and f3.launches == (Nout + 207) // 208
    rng = np.random.default_rng(K)
    A = (rng.standard_normal((M, K)) * np.exp(rng.uniform(-6, 6, (M, 1)))).astype(np.float32)   # wide dynamic range
    W = (rng.standard_normal((Nout, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(Nout).astype(np.float32)
    want = A.astype(np.float64) @ W.astype(np.float64).T + b
    Ad, Wd, bd = _to_dev(dev, A, W, b)
    got3 = ops.linear(Ad, Wd, bd, math=ops.MATH_BF16X3).cpu().numpy()
    got32 = ops.linear(Ad, Wd, bd, math=ops.MATH_FP32).cpu().numpy()
    scale = np.abs(A).astype(np.float64) @ np.abs(W).astype(np.float64).T + np.abs(b)      # sum |a||w|
    e3 = (np.abs(got3 - want) / scale).max()
    e32 = (np.abs(got32 - want) / scale).max()
    assert e3 <= 4e-7, (e3, e32)            # fp32 class: a few ulp of the absolute-value sum
    assert e3 <= 8 * max(e32, 6e-8), (e3, e32)


@pytest.mark.parametrize("path", [1, 2], ids=["unfused", "fused"])
@pytest.mark.parametrize("name", ["layer_d200.npz", "layer_d50.npz"])
def test_bf16x3_layer_stack_matches_reference_fixture(dev, bf16x3, name, path):
    from gnnrag_amd import stack
    cfg, batch, feats, params, ref = load_golden(name)
    out = stack.run_stack(batch, feats, params, dev, path=path)
    mask = batch.local_entity != batch.num_entity
    for c in range(cfg.T * cfg.L):
        dh = np.abs(out["h"][c] - ref["h"][c]).max()
        dd = np.abs(out["dist"][c] - ref["dist"][c]).max()
        ds = np.abs(out["score"][c][mask] - ref["score"][c][mask]).max() if mask.any() else 0.0
        assert dh <= TOL_INTERNAL and dd <= TOL_INTERNAL and ds <= TOL_INTERNAL, (c, dh, dd, ds)
        assert (out["dist"][c].argmax(1) == ref["dist"][c].argmax(1)).all()


def test_bf16x3_mid_size_vs_torch_cpu_oracle(dev, bf16x3):
    import oracle.rearev_torch_cpu as otorch
    from gnnrag_amd import stack, synth
    cfg = synth.GraphConfig(name="mid", B=4, N=2000, E=10000, R=600, D=200, I=2, L=3, T=2, seed=21)
    batch = synth.make_batch(cfg)
    feats = synth.make_features(cfg)
    params = synth.make_layer_params(cfg)
    want = otorch.run_stack(batch, feats, params)
    for path in (1, 2):
        got = stack.run_stack(batch, feats, params, dev, path=path)
        for c in range(cfg.T * cfg.L):
            assert np.abs(got["h"][c] - want["h"][c]).max() <= TOL_INTERNAL, (path, c)
            assert np.abs(got["dist"][c] - want["dist"][c]).max() <= TOL_INTERNAL, (path, c)
            assert (got["dist"][c].argmax(1) == want["dist"][c].argmax(1)).all()


def test_no_cpu_fallback_and_autograd_form_agrees(dev):
    """CPU tensors are refused (no fallback); with autograd enabled the layer takes its differentiable
    form (HIP aggregation + nn.Linear) and gives the same numbers as the fused inference call."""
    from gnnrag_amd import _lib, stack, synth
    cfg = synth.CONFIGS["tiny"]
    batch = synth.make_batch(cfg)
    feats = synth.make_features(cfg)
    params = synth.make_layer_params(cfg)
    devin = stack.DeviceInputs(batch, feats, dev)
    layer = stack.build_layer(cfg, batch, params, dev)
    stack.init_reason(layer, batch, devin, devin.h0)
    with torch.no_grad():
        want, _ = layer(devin.seed_dist, devin.ins[0], step=0)
    stack.init_reason(layer, batch, devin, devin.h0)
    with torch.enable_grad():
        got, _ = layer(devin.seed_dist, devin.ins[0], step=0)
    assert got.requires_grad and np.abs(got.detach().cpu().numpy() - want.cpu().numpy()).max() <= TOL_STATED
    with pytest.raises(_lib.GnnragError):
        from gnnrag_amd import ops
        ops.linear(torch.zeros(4, 4), torch.zeros(4, 4))


@pytest.mark.parametrize("B,N,D", [(3, 70, 50), (64, 2000, 200), (2, 130, 300), (20, 500, 200), (1, 2000, 50)])
def test_query_reform_seed_retrieve(dev, B, N, D):
    """QueryReform drop-in (query_update.py:26-44): the seed retrieval kernel against torch.bmm, and the
    module's output against fusion(q, bmm) with the same parameters (the reference's attention over all
    nodes does not enter its return value)."""
    from gnnrag_amd import ops
    from gnnrag_amd.modules.query_update import QueryReform
    g = torch.Generator().manual_seed(B + N)
    ent = torch.randn(B, N, D, generator=g).to(dev)
    seed = torch.zeros(B, N)
    seed[:, 0] = 1.0
    if B > 1:
        seed[1, N - 1] = 0.5                     # two seeds with fractional weights (seed_dist-style input)
        seed[1, 0] = 0.5
    if B > 2:
        seed[2] = 0.0                            # a question without a seed
    seed = seed.to(dev)
    want = torch.bmm(seed.unsqueeze(1), ent).squeeze(1)
    got = ops.seed_retrieve(seed, ent)
    assert torch.equal(got, want) or (got - want).abs().max().item() <= 1e-6
    torch.manual_seed(0)
    qr = QueryReform(D).to(dev).eval()
    q = torch.randn(B, D, generator=g).to(dev)
    with torch.no_grad():
        out = qr(q, ent, seed, (seed == 0).float())         # one launch: gnnrag_query_reform
        ref = qr.fusion(q, want)                            # the reference's Fusion on torch (query_update.py:6-16)
        assert (out - ref).abs().max().item() <= 4e-6       # two fp32 summation orders of 3 D terms (1.2e-6 seen at D = 200)
        # a node state kept zero-padded by ReasonGNNLayer (hidden size 50 -> 56): the view the caller holds carries its
        # padded base, which the kernel reads in place with the padded row stride
        Dp = (D + 7) // 8 * 8 + 8
        base = torch.zeros(B, N, Dp, device=dev)
        base[..., :D] = ent
        view = base[..., :D]
        view._gnnrag_padded = base
        assert torch.equal(qr(q, view, seed, (seed == 0).float()), out)
        assert torch.equal(ops.query_reform(q, seed, ent, qr.fusion.r.weight, qr.fusion.g.weight), out)


def test_query_reform_equals_reference_op_sequence_at_c2(dev, capsys):
    """C2-sized node state: the drop-in against the reference's full op sequence (incl. its unused attention
    over all nodes, restated in oracle/query_update_torch.py) run on the same GPU; prints both times."""
    import oracle.query_update_torch as oq
    from gnnrag_amd.modules.query_update import QueryReform
    B, N, D = 64, 2000, 200
    g = torch.Generator().manual_seed(1)
    ent = torch.randn(B, N, D, generator=g).to(dev)
    q = torch.randn(B, D, generator=g).to(dev)
    seed = torch.zeros(B, N)
    seed[:, 0] = 1.0
    seed = seed.to(dev)
    local_entity = torch.randint(0, 1000, (B, N), generator=g).to(dev)        # rearev.py:219 passes entity IDS as "mask"
    torch.manual_seed(0)
    qr = QueryReform(D).to(dev).eval()

    def ref():
        return oq.query_reform(q, ent, seed, local_entity, qr.q_ent_attn.weight, qr.q_ent_attn.bias,
                               qr.fusion.r.weight, qr.fusion.g.weight)

    def mine():
        return qr(q, ent, seed, local_entity)

    with torch.no_grad():
        # the drop-in is ONE launch (gnnrag_query_reform): its 600-term sums run in another fp32 order than hipBLASLt's
        # (1.6e-6 seen on values up to ~4, i.e. 3 ulp; the stated bar is 1e-4)
        assert (mine() - ref()).abs().max().item() <= 4e-6
        times = []
        for fn in (ref, mine):
            fn()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(10):
                fn()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) / 10)
    with capsys.disabled():
        print("\nQueryReform at C2: reference op sequence %.3f ms, drop-in %.3f ms" % tuple(times))


@pytest.mark.parametrize("B,R,used,I,N,D", [(4, 600, None, 2, 1200, 200), (9, 1500, 260, 3, 1500, 200),
                                            (3, 40, None, 1, 300, 200), (5, 500, None, 2, 1000, 208)])
def test_relation_tables_bf16x3_w_resident_kernel(dev, B, R, used, I, N, D):
    """The bf16x3 relation tables on the W-resident kernel (tables_b3.hip; D = 200, >= 1024 compact rows): against
    the exact-fp32 kernel and the float64 definition, incl. questions of very different relation counts (row chunks
    that span several questions), 1-3 instructions and a row count that is not a multiple of 16."""
    from gnnrag_amd import ops, synth
    cfg = synth.GraphConfig(name="tab", B=B, N=N, E=6 * N, R=R, D=D, I=I, L=1, T=1, seed=B + R, rel_per_question=used,
                            n_real_min=N // 3)
    batch = synth.make_batch(cfg)
    et = batch.edge_tuple
    plan = ops.CsrPlan(et[0], et[1], et[2], cfg.B, cfg.N, cfg.R1, dev)
    assert plan.rel_total >= 1024 or (B, R) == (3, 40)          # that case stays on the k-tiled kernel
    rng = np.random.default_rng(5)
    Tf = (0.3 * rng.standard_normal((cfg.R1, D))).astype(np.float32)
    Ti = (0.3 * rng.standard_normal((cfg.R1, D))).astype(np.float32)
    ins = (0.3 * rng.standard_normal((B, I, D))).astype(np.float32)
    W = rng.uniform(-0.05, 0.05, size=(D, (2 * I + 1) * D)).astype(np.float32)
    dTf, dTi, dins, dW = (torch.from_numpy(x).to(dev) for x in (Tf, Ti, ins, W))
    P32 = ops.relation_tables(plan, dTf, dTi, dins, dW, math=ops.MATH_FP32).cpu().numpy()
    Pb3 = ops.relation_tables(plan, dTf, dTi, dins, dW, math=ops.MATH_BF16X3).cpu().numpy()
    rows = plan.rel_rows()
    want = np.zeros((2, plan.rel_total, D))
    for d, Tt in enumerate((Tf, Ti)):
        for i in range(I):
            A = np.maximum(Tt[rows[:, 1]].astype(np.float64) * ins[rows[:, 0], i].astype(np.float64), 0.0)
            want[d] += A @ W[:, (1 + 2 * i + d) * D:(2 + 2 * i + d) * D].astype(np.float64).T
    scale = max(1.0, np.abs(want).max())
    assert np.abs(P32 - want).max() <= TOL_INTERNAL * scale
    assert np.abs(Pb3 - want).max() <= TOL_INTERNAL * scale


@pytest.mark.parametrize("B,R,used,I,N,D", [(4, 600, None, 2, 1200, 200), (9, 1500, 260, 3, 1500, 200),
                                            (64, 600, None, 2, 400, 200), (70, 900, 40, 1, 300, 200),
                                            (6, 700, None, 2, 900, 208)])
def test_relation_tables_from_relation_planes(dev, B, R, used, I, N, D):
    """The V form of the relation tables (k_tables_vq): relu(t q) = max(q,0) relu(t) + max(-q,0) relu(-t) moves the
    question into a per-question right operand and leaves [relu(T), relu(-T)] as a question-independent left operand
    whose bf16 planes the projection kernel writes.  Checks (1) the planes: hi + mid + lo == relu(+-T) EXACTLY,
    zero padding; (2) the tables against the float64 definition and the exact-fp32 kernel - few questions (row chunks
    per question), many questions, very different relation counts per question, 1-3 instructions."""
    from gnnrag_amd import ops, synth
    cfg = synth.GraphConfig(name="tabv", B=B, N=N, E=6 * N, R=R, D=D, I=I, L=1, T=1, seed=B + R, rel_per_question=used,
                            n_real_min=N // 3)
    batch = synth.make_batch(cfg)
    et = batch.edge_tuple
    plan = ops.CsrPlan(et[0], et[1], et[2], cfg.B, cfg.N, cfg.R1, dev)
    assert plan.rel_total >= 1024
    rng = np.random.default_rng(7)
    relf = [rng.standard_normal((cfg.R1, D)).astype(np.float32) for _ in range(2)]
    layers = []
    for j in range(2):
        Wr = (rng.standard_normal((D, D)) / np.sqrt(D) * 0.4).astype(np.float32)
        br = (0.1 * rng.standard_normal(D)).astype(np.float32)
        layers.append((torch.from_numpy(Wr).to(dev), torch.from_numpy(br).to(dev), None, None))
    T, planes = ops.rel_transform(torch.from_numpy(relf[0]).to(dev), torch.from_numpy(relf[1]).to(dev), layers, planes=True)
    Tn = T.cpu().numpy()
    pl = planes.cpu().numpy().view(np.uint16).astype(np.uint32)               # [L, 2, 3, R1, 448]
    as_f32 = (pl << 16).view(np.float32)
    total = as_f32[:, :, 0].astype(np.float64) + as_f32[:, :, 1] + as_f32[:, :, 2]
    assert np.array_equal(total[..., :D], np.maximum(Tn, 0).astype(np.float64))
    assert np.array_equal(total[..., 224:224 + D], np.maximum(-Tn, 0).astype(np.float64))
    assert not pl[..., D:224].any() and not pl[..., 224 + D:].any()
    ins = (0.3 * rng.standard_normal((B, I, D))).astype(np.float32)
    W = rng.uniform(-0.05, 0.05, size=(D, (2 * I + 1) * D)).astype(np.float32)
    dins, dW = torch.from_numpy(ins).to(dev), torch.from_numpy(W).to(dev)
    rows = plan.rel_rows()
    for j in (1, 0):
        Pv = ops.relation_tables_planes(plan, planes[j], dins, dW).cpu().numpy()
        P32 = ops.relation_tables(plan, T[j, 0], T[j, 1], dins, dW, math=ops.MATH_FP32).cpu().numpy()
        want = np.zeros((2, plan.rel_total, D))
        for d in range(2):
            for i in range(I):
                A = np.maximum(Tn[j, d][rows[:, 1]].astype(np.float64) * ins[rows[:, 0], i].astype(np.float64), 0.0)
                want[d] += A @ W[:, (1 + 2 * i + d) * D:(2 + 2 * i + d) * D].astype(np.float64).T
        scale = max(1.0, np.abs(want).max())
        assert np.abs(Pv - want).max() <= TOL_INTERNAL * scale
        assert np.abs(P32 - want).max() <= TOL_INTERNAL * scale


@pytest.mark.parametrize("M", [9000, 8192, 16000, 9008])
@pytest.mark.parametrize("D", [200, 208])
def test_update_bf16x3_w_resident_vs_exact_fp32(dev, M, D):
    """k_update_b3 against the exact-fp32 kernel on random data at both hidden sizes it admits.  Regression: at
    D = 208 the 6-tile column part ends at its last staged LDS row, and the last k block of column 207 read 32 bytes of
    an UNWRITTEN row behind it - 0 x stale Inf/NaN = NaN, relu -> 0 for some rows (b3_tile.h: tab_stage_rows)."""
    from gnnrag_amd import ops
    g = torch.Generator(device="cpu").manual_seed(M + D)
    r = lambda *shape: torch.randn(*shape, generator=g).to(dev)
    h, nbr, W, b, ws, bs = r(M, D), r(M, D), r(D, 5 * D) / 14, r(D), r(D), r(1)
    mask = (torch.rand(M, generator=g) > 0.1).float().to(dev)
    h32, s32 = ops.update_score_fused(h, nbr, W, b, ws, bs, mask, 2, math=ops.MATH_FP32)
    hb3, sb3 = ops.update_score_fused(h, nbr, W, b, ws, bs, mask, 2, math=ops.MATH_BF16X3)
    assert float((h32 - hb3).abs().max()) <= 2e-5 * max(1.0, float(h32.abs().max()))
    live = mask > 0
    assert float((s32 - sb3)[live].abs().max()) <= 1e-4 * max(1.0, float(s32[live].abs().max()))
    assert torch.equal(s32[~live], sb3[~live])                        # masked slots: exactly -1e11 in both


@pytest.mark.parametrize("direction", [0, 1], ids=["fwd", "inv"])
def test_one_direction_layer_skips_the_other_direction(dev, direction, capsys):
    """NSM layers aggregate along ONE direction (nsm_gnn.py:87-112 / :118-142): with GNNRAG_PATH_ONLY_FWD / _INV only
    that direction's relation tables are built (V form) and walked (LDS walk).  Same results as the both-direction
    call with a zero weight block for the other direction, which is what small / odd shapes still run."""
    from gnnrag_amd import _lib, ops, stack, synth
    cfg = synth.GraphConfig(name="nsm1d", B=16, N=2000, E=10000, R=600, D=200, I=1, L=1, T=1, seed=31 + direction)
    batch = synth.make_batch(cfg)
    feats = synth.make_features(cfg)
    params = synth.make_layer_params(cfg)
    devin = stack.DeviceInputs(batch, feats, dev)
    et = batch.edge_tuple
    plan = ops.CsrPlan(et[0], et[1], et[2], cfg.B, cfg.N, cfg.R1, dev)
    assert ops.aggregate_fused_variant(plan, cfg.D) != ops.WALK_L2_GATHER and plan.rel_total >= 1024
    D = cfg.D
    P = {k: torch.from_numpy(v).to(dev) for k, v in params.items()}
    W = P["e2e_linear0.weight"].clone()                               # [D, 3D]: self | fwd | inv
    W[:, (2 - direction) * D:(3 - direction) * D] = 0                 # the direction that is not walked
    mask = torch.ones(cfg.B, cfg.N, device=dev)
    args = (plan, devin.h0, devin.seed_dist, devin.ins[0], devin.rel_features, devin.rel_features_inv,
            P["rel_linear0.weight"], P["rel_linear0.bias"], W, P["e2e_linear0.bias"], P["score_func.weight"],
            P["score_func.bias"], mask)
    flag = _lib.PATH_ONLY_INV if direction else _lib.PATH_ONLY_FWD
    both = ops.reason_layer(*args, path=_lib.PATH_FUSED)
    one = ops.reason_layer(*args, path=_lib.PATH_FUSED | flag)
    # equal up to the summation order in hub rows: the both-direction call walks a node's facts of both directions as one
    # merged run (the zero block's facts add exact zeros, but the wave-per-hub partial sums group differently)
    for a, b in zip(both, one):
        assert float((a - b).abs().max()) <= 2e-6 * max(1.0, float(a.abs().max()))
    assert torch.equal(both[2].argmax(1), one[2].argmax(1))
    import bench
    t_both = float(np.mean(bench._events_ms(lambda: ops.reason_layer(*args, path=_lib.PATH_FUSED), 10)))
    t_one = float(np.mean(bench._events_ms(lambda: ops.reason_layer(*args, path=_lib.PATH_FUSED | flag), 10)))
    with capsys.disabled():
        print("\none-direction layer (B=16, N=2000, D=200): both directions %.3f ms, one %.3f ms" % (t_both, t_one))
    with pytest.raises(_lib.GnnragError):
        ops.reason_layer(*args, path=_lib.PATH_FUSED | _lib.PATH_ONLY_FWD | _lib.PATH_ONLY_INV)


@pytest.mark.parametrize("cfgname", ["tiny50", "mid", "C2"])
def test_whole_iteration_call_and_graph_replay_are_bit_identical(dev, cfgname):
    """f-3: the L layer calls of a ReaRev iteration as ONE library call (gnnrag_reason_stack, run ahead by the module's
    step-0 call) and as a replayed hipGraph (gnnrag_reason_stack_capture) reproduce the per-layer calls bit for bit -
    every layer's h / score / dist, over T iterations with carried node state and changing instructions."""
    from gnnrag_amd import ops, stack, synth
    if cfgname == "mid":
        cfg = synth.GraphConfig(name="mid", B=4, N=2000, E=10000, R=600, D=200, I=2, L=3, T=3, seed=21)
    elif cfgname == "C2":
        cfg = synth.GraphConfig(**{**synth.CONFIGS["C2"].__dict__, "T": 2})
    else:
        cfg = synth.GraphConfig(**{**synth.CONFIGS["tiny50"].__dict__, "T": 3})
    batch = synth.make_batch(cfg)
    feats = synth.make_features(cfg)
    params = synth.make_layer_params(cfg)
    devin = stack.DeviceInputs(batch, feats, dev)
    outs = {}
    for mode in ("per_layer", "stack"):
        layer = stack.build_layer(cfg, batch, params, dev)
        layer.use_stack = mode == "stack"
        stack.init_reason(layer, batch, devin, devin.h0)
        _, rec = stack.run_layers(layer, cfg, devin, record=True)
        outs[mode] = rec
        if mode == "stack":
            assert layer._stack is not None and layer._ahead is not None          # the run-ahead path really ran
    for k in ("h", "score", "dist"):
        for a, b in zip(outs["per_layer"][k], outs["stack"][k]):
            assert np.array_equal(a, b), k
    # graph replay over fixed buffers: node state carried in h[L-1], instructions rewritten in place.  The module pads
    # hidden sizes that are not a multiple of 4 (tiny50: 50 -> 56): the explicit stack gets the same padded operands.
    import torch.nn.functional as F
    layer = stack.build_layer(cfg, batch, params, dev)
    stack.init_reason(layer, batch, devin, devin.h0)
    with torch.no_grad():
        P = layer._inference_params()
        D, Dp = P["D"], P["Dp"]
        pad = (lambda t: t if Dp == D else F.pad(t, (0, Dp - D)))
        # (same path word as the module's own stack: layer 0 takes the seed-prior form, csrc/frontier.hip)
        st = ops.LayerStack(layer.plan, P["relfeat"], P["relfeat_inv"], P["layers"], P["w_score"], P["b_score"],
                            layer.local_entity_mask, cfg.I, path=layer._path_of(0))
        st.run(pad(devin.h0), devin.seed_dist, pad(devin.ins[0]))                 # eager once (launch attributes)
        ins_buf = pad(devin.ins[0]).clone()
        st.capture(pad(devin.h0), devin.seed_dist, ins_buf)
        c = 0
        for t in range(cfg.T):
            ins_buf.copy_(pad(devin.ins[t]))
            h, score, dist = st.replay(first=(t == 0))      # iterations 2..T: the graph without the relation projections
            for j in range(cfg.L):
                assert np.array_equal(h[j][..., :D].cpu().numpy(), outs["per_layer"]["h"][c])
                assert (h[j][..., D:] == 0).all()                                 # padded columns stay exactly zero
                assert np.array_equal(dist[j].cpu().numpy(), outs["per_layer"]["dist"][c])
                assert np.array_equal(score[j].cpu().numpy(), outs["per_layer"]["score"][c])
                c += 1
        st.release_graph()
