"""Float64 oracle of the training loss (``gnnrag_kl_loss_train`` / ``gnnrag_kl_loss_backward``), a plain-Python restatement of
the batch metrics (``gnnrag_train_metrics``: what ``calc_h1``, ``calc_f1_new`` and ``f1_and_hits`` of the reference's
``base_model.py`` compute), and the generator of their cases.

The restatement is written from the description of those functions, over Python floats (doubles) converted from the fp32
inputs, the way ``.tolist()`` hands them to the reference's loop.  tests/golden/train_tail_ref.npz holds what the live
reference returned for ``FIXTURE_CASES``; tests/test_train_tail_host.py holds this file to it."""
import numpy as np

PAD_ID = 100000
KINDS = 9
FIXTURE_CASES = {"n8": (9, 8, 0, 0.95), "n8e3": (9, 8, 0, 0.3), "n64": (9, 64, 3, 0.95), "n67e3": (9, 67, 5, 0.3)}   # B, N, seed, eps


# -- the loss ---------------------------------------------------------------------------------------------------------------

def loss_and_grad(pred, teacher, label_valid, g=1.0):
    """float64: (loss, d_pred [B,N], len [B], l [B]) of calc_loss_label with the KL loss; g the upstream gradient.  The one
    fp32 addition ``pred + 1e-8`` (base_model.py:197) is taken as the reference makes it - its fp32 result is the argument of
    the logarithm (at pred = 1 it is 1, not 1 + 1e-8) - and everything after it is float64."""
    p, t = np.asarray(pred, np.float64), np.asarray(teacher, np.float64)
    lv = np.asarray(label_valid, np.float64).reshape(-1)
    B = p.shape[0]
    ln = t.sum(1)
    ln[ln == 0] = 1.0
    th = t / ln[:, None]
    q = (np.asarray(pred, np.float32) + np.float32(1e-8)).astype(np.float64)
    pos = th > 0
    terms = np.zeros_like(p)
    terms[pos] = th[pos] * (np.log(th[pos]) - np.log(q[pos]))
    l = lv * terms.sum(1)
    d = np.where(pos, -float(g) * lv[:, None] * th / q / B, 0.0)
    return l.sum() / B, d, ln, l


# -- the metrics ------------------------------------------------------------------------------------------------------------

def question_metrics(probs, answer, seed, ents, pad_id, eps):
    """One question, everything a Python float / int.  Returns (argmax, h1, f1 before the H@1 gate, (kept, n_ret, correct,
    n_ans), precision, recall)."""
    N = len(probs)
    top = 0
    for j in range(1, N):
        if probs[j] > probs[top]:
            top = j                                   # the first of equal maxima stays
    h1 = 1.0 if answer[top] > float(np.float32(1e-10)) else 0.0
    ignore = (1 - eps) / N
    answers, kept = [], []
    for j in range(N):
        if seed[j] > 0 or ents[j] == pad_id:
            continue
        if answer[j] > 0:
            answers.append(ents[j])
        if probs[j] < ignore:
            continue
        kept.append((ents[j], probs[j]))
    ranked = sorted(kept, key=lambda cp: cp[1], reverse=True)          # stable: equal probabilities keep slot order
    total, n_ret, correct = 0.0, 0, 0
    for ent, prob in ranked:
        n_ret += 1
        total += prob
        if ent in answers:
            correct += 1
        if total > eps:
            break
    if not answers:
        pr, rc, f1 = (1.0, 1.0, 1.0) if n_ret == 0 else (0.0, 1.0, 0.0)
    elif n_ret == 0:
        pr, rc, f1 = 1.0, 0.0, 0.0
    else:
        pr, rc = correct / n_ret, correct / len(answers)
        f1 = 2.0 / (1.0 / pr + 1.0 / rc) if pr != 0 and rc != 0 else 0.0
    return top, h1, f1, (len(kept), n_ret, correct, len(answers)), pr, rc


def metrics(pred, answer, seed, local_entity, pad_id, eps):
    """The batch: dict of ``pred`` int32 [B], ``h1`` / ``f1`` float32 [B] (f1 gated by h1, rounded to fp32 once), ``cnt``
    int32 [B,4], and the ungated ``f1_raw`` / ``precision`` / ``recall`` float64 [B]."""
    B = pred.shape[0]
    out = {"pred": np.zeros(B, np.int32), "h1": np.zeros(B, np.float32), "f1": np.zeros(B, np.float32),
           "cnt": np.zeros((B, 4), np.int32), "f1_raw": np.zeros(B), "precision": np.zeros(B), "recall": np.zeros(B)}
    for b in range(B):
        top, h1, f1, cnt, pr, rc = question_metrics(pred[b].tolist(), answer[b].tolist(), seed[b].tolist(),
                                                    local_entity[b].tolist(), pad_id, eps)
        out["pred"][b], out["h1"][b], out["cnt"][b] = top, h1, cnt
        out["f1"][b] = np.float32(f1) if h1 else np.float32(0.0)
        out["f1_raw"][b], out["precision"][b], out["recall"][b] = f1, pr, rc
    return out


# -- the cases --------------------------------------------------------------------------------------------------------------

def _question(rng, N, kind, eps):
    """One question of N slots.  ``kind`` picks the corner it is built around (see ``case``)."""
    n_pad = min(N // 4, 100)
    live = N - n_pad
    logits = 4.0 * rng.standard_normal(N)
    p = np.exp(logits - logits.max())
    p = (p / p.sum()).astype(np.float32)
    ents = np.full(N, PAD_ID, np.int64)
    ents[:live] = rng.permutation(PAD_ID)[:live]                 # distinct ids, as the batch builder guarantees
    seed, ans = np.zeros(N, np.float32), np.zeros(N, np.float32)
    s = int(rng.integers(live))
    seed[s] = 1.0
    others = [j for j in range(live) if j != s]
    tiny = np.float32((1 - eps) / N / 8)                         # below ignore_prob
    if kind == 0:                                                # a hit: the argmax is an eligible answer
        top = int(np.argmax(p))
        if (top >= live or top == s) and others:
            p[top], p[others[0]] = p[others[0]], p[top]
            top = others[0]
        if top < live and top != s:
            ans[top] = 1.0
        for j in rng.permutation(others)[:2]:
            ans[j] = 1.0
    elif kind == 1:                                              # no answers: label_valid = 0, len replaced by 1
        pass
    elif kind == 2:                                              # pad slots only; the argmax carries an answer flag
        ents[:] = PAD_ID
        ans[int(np.argmax(p))] = 1.0
    elif kind == 3:                                              # the argmax is a seed that is an answer; the rest is retrieved
        p[s] = np.float32(p.max() * 2)
        ans[s] = 1.0
    elif kind in (4, 5):                                         # ... and nothing eligible survives ignore_prob
        p[:] = tiny
        p[s] = np.float32(0.97)
        ans[s] = 1.0
        if kind == 5 and others:                                 # with an eligible answer: f1_and_hits returns 1, 0, 0, hits
            ans[others[0]] = 1.0
    elif kind == 6:                                              # exact ties at the argmax and inside the prefix, zeros behind
        seed[:] = 0.0
        p[:] = 0.0
        pattern = [0.25, 0.25, 0.25, 0.125, 0.125]
        p[:min(live, 5)] = pattern[:min(live, 5)]                # sums to exactly 1.0: the cut is the last kept slot
        ans[0] = 1.0
        if live > 2:
            ans[2] = 1.0
        if live > 5:
            seed[5] = 1.0
    elif kind == 7:                                              # the running sum never exceeds a large eps
        p[:] = tiny
        p[s] = np.float32(0.4)
        if others:
            p[others[0]] = np.float32(0.45)
            ans[others[0]] = 1.0
            for j in others[1:4]:
                p[j] = np.float32(0.03)
                ans[j] = float(j % 2)
        else:
            ans[s] = 1.0
    else:                                                        # zeros in pred, a tie of the two largest, a weighted teacher
        if len(others) >= 2:
            a, b = sorted(others[:2])
            p[a] = p[b] = p.max()
            ans[a], ans[b] = 0.5, 2.0
        for j in others[2:5]:
            p[j] = 0.0
    return p, ans, seed, ents


def case(B, N, seed=0, eps=0.95):
    """A batch whose question b is built around corner ``(seed + b) % KINDS``: 0 a plain hit, 1 no answers, 2 pad slots only,
    3 / 4 the argmax is a seed that is an answer with a non-empty / an empty retrieved list, 5 nothing eligible survives
    ignore_prob although there are answers, 6 exact ties at the argmax and in the prefix with the cut on the last kept slot
    and zeros in pred, 7 a running sum that never exceeds eps = 0.95, 8 zeros, a tie of the two largest and a weighted
    teacher.  teacher = answer (rearev.py:233); every answer slot has pred > 0."""
    rng = np.random.default_rng(1000 * seed + 7 * N + B)
    rows = [_question(rng, N, (seed + b) % KINDS, eps) for b in range(B)]
    pred, answer, sd, ents = (np.stack([r[i] for r in rows]) for i in range(4))
    assert not ((answer > 0) & (pred == 0)).any()
    for b in range(B):
        live = ents[b][ents[b] != PAD_ID]
        assert len(set(live.tolist())) == len(live)
    valid = (answer.sum(1, keepdims=True) > 0).astype(np.float32)
    return {"pred": pred, "answer": answer, "teacher": answer.copy(), "label_valid": valid, "seed": sd,
            "local_entity": ents, "pad_id": PAD_ID, "eps": float(eps), "g": np.float32(0.75 + 0.5 * rng.random())}


def timing_case(B, N, hit_share, seed=0, eps=0.95):
    """The measurement's inputs: a softmax of 4 N(0,1) logits, 100 pad slots, one seed per question, three answers; the first
    ``round(hit_share * B)`` questions have H@1 = 1 (an answer at the argmax), the others none."""
    rng = np.random.default_rng(seed)
    n_pad = min(100, N // 4)
    live = N - n_pad
    logits = 4.0 * rng.standard_normal((B, N))
    logits[:, live:] = -30.0
    p = np.exp(logits - logits.max(1, keepdims=True))
    pred = (p / p.sum(1, keepdims=True)).astype(np.float32)
    ents = np.full((B, N), PAD_ID, np.int64)
    seed_d, ans = np.zeros((B, N), np.float32), np.zeros((B, N), np.float32)
    hits = int(round(hit_share * B))
    for b in range(B):
        ents[b, :live] = rng.permutation(PAD_ID)[:live]
        top = int(np.argmax(pred[b]))
        free = [j for j in range(live) if j != top]
        picks = rng.permutation(free)[:4]
        seed_d[b, picks[0]] = 1.0
        ans[b, picks[1:]] = 1.0
        if b < hits:
            ans[b, top] = 1.0
    valid = (ans.sum(1, keepdims=True) > 0).astype(np.float32)
    return {"pred": pred, "answer": ans, "teacher": ans.copy(), "label_valid": valid, "seed": seed_d, "local_entity": ents,
            "pad_id": PAD_ID, "eps": float(eps), "g": np.float32(1.0)}


# -- a stand-in model ---------------------------------------------------------------------------------------------------------

class StandIn:
    """What ``patch_loss_metrics`` wraps, without the reference at hand: ``calc_loss_label`` is the torch expression of
    rearev.py:156-160 over base_model.py:187-215 (autograd works through it), ``get_eval_metric`` the restatement above
    behind the host copies the reference makes.  ``calls`` counts what reached these methods."""

    def __init__(self, c, device="cpu", loss_type="kl"):
        import torch
        self.loss_type, self.eps, self.num_entity, self.device = loss_type, c["eps"], c["pad_id"], torch.device(device)
        self.seed_entities = torch.from_numpy(c["seed"]).to(self.device).requires_grad_(True)        # rearev.py:175
        self.local_entity = torch.from_numpy(c["local_entity"]).to(self.device)
        self.calls = {"loss": 0, "metric": 0}

    def calc_loss_label(self, curr_dist, teacher_dist, label_valid):
        import torch
        import torch.nn.functional as F
        self.calls["loss"] += 1
        if self.loss_type == "bce":
            tp = F.binary_cross_entropy_with_logits(curr_dist, (teacher_dist > 0).float() * 0.9, reduction="none")
        else:
            ln = torch.sum(teacher_dist, dim=1, keepdim=True)
            ln = torch.where(ln == 0, torch.ones_like(ln), ln)
            tp = F.kl_div(torch.log(curr_dist + 1e-8), teacher_dist.div(ln), reduction="none")
        return torch.sum(tp * label_valid) / curr_dist.size(0)

    def get_eval_metric(self, pred_dist, answer_dist):
        import torch
        self.calls["metric"] += 1
        m = metrics(pred_dist.detach().cpu().numpy(), answer_dist.detach().cpu().numpy(),
                    self.seed_entities.detach().cpu().numpy(), self.local_entity.cpu().numpy(), self.num_entity, self.eps)
        return torch.from_numpy(m["h1"]).to(self.device), torch.from_numpy(m["f1"]).to(self.device)
