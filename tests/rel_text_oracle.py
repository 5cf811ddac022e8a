"""float64 oracle of the relation-text branch of ``get_rel_feature`` (reference ``models/ReaRev/rearev.py:101-106``,
``models/NSM/nsm.py:103-105`` with ``modules/query_update.py:46-61``) and of its autograd gradients - the reference's
expression as it is written, NOT the collapsed form the kernels use:

    h = X W^T + b;  s = h a;  s' = s - (1 - mask) * 1e8;  alpha = softmax_t(s');  out = sum_t alpha_t h_t

One thing is taken from fp32 on purpose: the mask offset.  ``s - 1e8`` in fp32 rounds to a multiple of 8, and a row of
padding only (``rel_texts`` has them by construction, ``dataset_load.py:413-423``) gets the softmax of these ROUNDED values
- exactly uniform while |s| < 4.  The oracle applies the offset to ``float32(s)`` in fp32 and carries the result on in
float64 (the gradient passes through as for the plain difference).  Test infrastructure only."""
import numpy as np
import torch

MASK_OFF = 1e8
QUANTITIES = ("out", "dW", "db", "da")


def masked_scores(s, mask):
    """s [R,T] float64 -> s - (1 - mask) 1e8 with the offset applied in fp32; tokens (mask == 1) keep s exactly."""
    q = (s.detach().float() - (1 - mask.float()) * MASK_OFF).double()
    return torch.where(mask == 1, s, s + (q - s.detach()))


def pool64(X, mask, W, b, a):
    """One direction in float64 torch (differentiable in W, b, a): returns (out [R,D], alpha [R,T], s [R,T])."""
    h = X @ W.t() + b
    s = h @ a
    alpha = torch.softmax(masked_scores(s, mask), dim=1)
    return (h * alpha[:, :, None]).sum(1), alpha, s


def pool32(X, mask, W, b, a):
    """The same expression in torch fp32 ops, the way the reference evaluates it: its own rounding error."""
    h = torch.nn.functional.linear(X, W, b)
    s = torch.nn.functional.linear(h, a[None, :])
    s = s - (1 - mask[:, :, None]) * MASK_OFF
    return (h * torch.softmax(s, dim=1)).sum(1)


def _run(fn, dtype, Xs, mask, W, b, a, gs):
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dtype)      # noqa: E731
    Wt, bt, at = (t(v).requires_grad_(True) for v in (W, b, a.reshape(-1)))
    outs = [fn(t(X), t(mask), Wt, bt, at) for X in Xs]
    outs = [o[0] if isinstance(o, tuple) else o for o in outs]
    loss = sum((o * t(g)).sum() for o, g in zip(outs, gs) if g is not None)
    dW, db, da = torch.autograd.grad(loss, (Wt, bt, at))
    return dict(out=[o.detach().numpy() for o in outs], dW=dW.numpy(), db=db.numpy(), da=da.numpy())


def oracle(Xs, mask, W, b, a, gs):
    """Xs: the directions' token states (1 or 2 arrays [R,T,K]), gs: their upstream gradients [R,D] (None = zeros).
    Returns dict(out=[per direction], dW, db, da) in float64; both directions share W, b, a and the mask."""
    return _run(pool64, torch.float64, Xs, mask, W, b, a, gs)


def reference32(Xs, mask, W, b, a, gs):
    """The reference's fp32 evaluation (torch CPU) of the same quantities."""
    return _run(pool32, torch.float32, Xs, mask, W, b, a, gs)


def scores(X, mask, W, b, a):
    """float64 scores s [R,T] before the mask offset, and which rows are padding only."""
    s = (X.astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64)) @ a.astype(np.float64).reshape(-1)
    return s, mask.sum(1) == 0


def rel_err(got, want):
    """Largest error relative to the largest entry of the oracle's result."""
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


def errors(got, want):
    """{quantity: rel_err}; 'out' is the worst direction."""
    e = {q: rel_err(got[q], want[q]) for q in ("dW", "db", "da")}
    e["out"] = max(rel_err(g, w) for g, w in zip(got["out"], want["out"]))
    return e


def random_case(R, T, K, D, seed=0, n_dir=2, a_scale=0.5):
    """Inputs with rows of no token, one token and T tokens; the scale of ``a`` keeps |s| well below 3.5 (s ~ N(0,
    a_scale^2)), so that rows of padding only get the uniform weights.  fp32 arrays."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, T + 1, R)
    lens[0] = T
    if R > 1:
        lens[-1] = 0
    if R > 2:
        lens[1] = 1
    if R > 3:
        lens[R // 2] = 0
    mask = (np.arange(T)[None, :] < lens[:, None]).astype(np.float32)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)      # noqa: E731
    return dict(Xs=[f(R, T, K) for _ in range(n_dir)], mask=mask, W=f(D, K) / np.float32(np.sqrt(K)),
                b=np.float32(0.1) * f(D), a=np.float32(a_scale / np.sqrt(D)) * f(1, D), gs=[f(R, D) for _ in range(n_dir)])


def fixture_case(z, tag):
    """One recorded case of tests/golden/rel_text_ref.npz as random_case lays it out, plus the recorded results."""
    g = lambda k: z["%s.%s" % (tag, k)]      # noqa: E731
    c = dict(Xs=[g("X_fwd"), g("X_inv")], mask=g("mask"), W=g("W"), b=g("b"), a=g("a"), gs=[g("g_fwd"), g("g_inv")])
    want = {"two": dict(out=[g("out_fwd"), g("out_inv")], dW=g("dW2"), db=g("db2"), da=g("da2")),
            "one": dict(out=[g("out_nsm")], dW=g("dW1"), db=g("db1"), da=g("da1"))}
    ref_err = {n: {q: float(g("err%s.%s" % (n, q))) for q in QUANTITIES} for n in ("1", "2")}
    return c, want, ref_err


FIXTURE_CASES = {"r37": (37, 5, 20, 12), "r24": (24, 9, 384, 50), "r5": (5, 1, 4, 1)}
PAD = 0


def make_standin(R1, T, K, D, directions=2, seed=0, device="cpu", lm="sbert"):
    """A model-like module with what ``patch_rel_feature`` needs (``rel_texts``, ``rel_features(_inv)``, ``lm``,
    ``instruction.question_emb`` / ``.pad_val``, ``self_att_r`` - the repo's own ``AttnEncoder``) and its OWN torch
    statement of ``get_rel_feature`` for the relation-text branch: a pair for ``directions == 2`` (ReaRev), one tensor for
    1 (NSM).  Token ids: rows of no token, one token and T tokens, padded with ``PAD``."""
    import torch.nn as nn
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd.modules.query_update import AttnEncoder

    c = random_case(R1, T, K, D, seed=seed)
    gen = torch.Generator().manual_seed(seed)

    class Instruction(nn.Module):
        def __init__(self):
            super().__init__()
            self.question_emb = nn.Linear(K, D)
            self.pad_val = PAD

    class StandIn(nn.Module):
        def __init__(self):
            super().__init__()
            self.lm, self.num_relation = lm, R1 - 1
            self.instruction = Instruction()
            self.self_att_r = AttnEncoder(D)
            self.relation_embedding = nn.Embedding(R1, 4)
            self.relation_embedding_inv = nn.Embedding(R1, 4)
            self.relation_linear = nn.Linear(4, D)
            ids = torch.randint(1, 30, (R1, T), generator=gen)
            self.rel_texts = torch.where(torch.from_numpy(c["mask"]) == 1, ids, torch.full_like(ids, PAD))
            self.rel_texts_inv = self.rel_texts.clone()
            self.rel_features = torch.from_numpy(c["Xs"][0])
            self.rel_features_inv = torch.from_numpy(c["Xs"][1])
            self.calls = 0
            with torch.no_grad():
                self.self_att_r.attn_linear.weight.copy_(torch.from_numpy(c["a"]))

        def _apply(self, fn, *a, **k):
            super()._apply(fn, *a, **k)
            for n in ("rel_texts", "rel_texts_inv", "rel_features", "rel_features_inv"):
                if getattr(self, n) is not None:
                    setattr(self, n, fn(getattr(self, n)))
            return self

        def get_rel_feature(self):
            self.calls += 1
            if self.rel_texts is None:
                f = self.relation_linear(self.relation_embedding.weight)
                return (f, self.relation_linear(self.relation_embedding_inv.weight)) if directions == 2 else f
            mask = (self.rel_texts != self.instruction.pad_val).float()
            f = self.self_att_r(self.instruction.question_emb(self.rel_features), mask)
            if directions == 2:
                f_inv = self.self_att_r(self.instruction.question_emb(self.rel_features_inv), mask)
            if self.lm == "lstm":
                f = self.self_att_r(f, (self.rel_texts != self.num_relation + 1).float())
            return (f, f_inv) if directions == 2 else f

    return StandIn().to(device)


def standin_case(mod, directions=2):
    """The numpy operands of a stand-in as ``oracle`` takes them (without upstream gradients)."""
    c = lambda t: t.detach().cpu().numpy()      # noqa: E731
    Xs = [c(mod.rel_features)] + ([c(mod.rel_features_inv)] if directions == 2 else [])
    return dict(Xs=Xs, mask=c((mod.rel_texts != mod.instruction.pad_val).float()), W=c(mod.instruction.question_emb.weight),
                b=c(mod.instruction.question_emb.bias), a=c(mod.self_att_r.attn_linear.weight))
