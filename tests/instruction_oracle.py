"""Float64 numpy restatement of the instruction steps (reference gnn/modules/question_encoding/base_encoder.py:82-101),
shared by tests/test_instruction_host.py and tests/test_gpu_instruction*.py:

    q_s  = W_q[s] node + b_q[s]
    cq   = W_cq [r, q_s, q_s - r, q_s * r] + b_cq
    ca_t = w_ca . (cq * hidden[t]) + b_ca
    a    = softmax_t(ca_t + (1 - mask_t) * VERY_NEG)
    r    = sum_t a_t hidden[t]

The reference adds ``(1 - mask) * -1e11`` in fp32: for any |ca| < 4096 (half an ulp of 1e11 in fp32) the sum IS -1e11, so
here a padded token's logit is that constant.  A question of padding only therefore gets the uniform 1/T.  Also holds the
stand-in encoder module of the module tests and the input generator of the sweeps."""
import numpy as np

VERY_NEG = -100000000000.0


def instructions(hidden, node, mask, W_q, b_q, W_cq, b_cq, w_ca, b_ca, r_in=None):
    """hidden [B,T,D], node [B,D], mask [B,T] of 0 / 1, W_q / b_q lists -> (ins [n,B,D], attn [n,B,T]) in float64."""
    f = lambda a: np.asarray(a, dtype=np.float64)       # noqa: E731
    hidden, node, mask, W_cq, b_cq = f(hidden), f(node), f(mask), f(W_cq), f(b_cq)
    w_ca, b_ca = f(w_ca).reshape(-1), float(f(b_ca).reshape(-1)[0])
    B, T, D = hidden.shape
    r = np.zeros((B, D)) if r_in is None else f(r_in)
    ins, attn = [], []
    for W, b in zip(W_q, b_q):
        q = node @ f(W).T + f(b)
        cq = np.concatenate([r, q, q - r, q * r], axis=1) @ W_cq.T + b_cq
        ca = np.einsum("d,bd,btd->bt", w_ca, cq, hidden) + b_ca
        assert np.abs(ca).max() < 4096.0
        logit = np.where(mask != 0, ca, VERY_NEG)
        e = np.exp(logit - logit.max(axis=1, keepdims=True))
        a = e / e.sum(axis=1, keepdims=True)
        r = np.einsum("bt,btd->bd", a, hidden)
        ins.append(r)
        attn.append(a)
    return np.stack(ins), np.stack(attn)


def fixture_case(g, tag):
    """Inputs, parameters and the live reference's results of one tag of tests/golden/lstm_encoder.npz."""
    P = {k.split(".param.")[1]: g[k] for k in g.files if k.startswith(tag + ".param.")}
    text = g[tag + ".query_text"]
    hidden = g[tag + ".query_hidden_emb"]
    B, T, D = hidden.shape
    n = g[tag + ".instructions"].shape[0]
    return dict(hidden=hidden, node=g[tag + ".query_node_emb"].reshape(B, D),
                mask=(text != int(text.max())).astype(np.float32),          # the pad word is the largest id (num_word)
                W_q=[P["question_linear%d.weight" % i] for i in range(n)],
                b_q=[P["question_linear%d.bias" % i] for i in range(n)],
                W_cq=P["cq_linear.weight"], b_cq=P["cq_linear.bias"], w_ca=P["ca_linear.weight"], b_ca=P["ca_linear.bias"],
                want_ins=g[tag + ".instructions"], want_attn=g[tag + ".attn"].reshape(n, B, T))


def random_case(B, T, D, n, seed):
    """Weights drawn as nn.Linear initialises them (uniform +-1/sqrt(fan_in)), hidden states in (-1, 1), ragged masks:
    question 0 without padding, the last question (when B > 1) padding only."""
    rng = np.random.default_rng(seed)
    u = lambda shape, fan: rng.uniform(-1.0, 1.0, shape).astype(np.float32) / np.float32(np.sqrt(fan))   # noqa: E731
    lens = rng.integers(1, T + 1, B)
    lens[0] = T
    if B > 1:
        lens[-1] = 0
    mask = (np.arange(T)[None, :] < lens[:, None]).astype(np.float32)
    return dict(hidden=np.tanh(rng.standard_normal((B, T, D))).astype(np.float32),
                node=np.tanh(rng.standard_normal((B, D))).astype(np.float32), mask=mask,
                W_q=[u((D, D), D) for _ in range(n)], b_q=[u((D,), D) for _ in range(n)],
                W_cq=u((D, 4 * D), 4 * D), b_cq=u((D,), 4 * D), w_ca=u((1, D), D), b_ca=u((1,), D))


ARGS = ("hidden", "node", "mask", "W_q", "b_q", "W_cq", "b_cq", "w_ca", "b_ca")


def make_standin(word_dim, entity_dim, num_ins, num_word, linear_dropout=0.0, device="cpu"):
    """A module with the attributes ``patch_instruction`` needs and its OWN torch statement of the steps - written for
    these tests, with an LSTM encoder, so that the module tests do not depend on the staged reference."""
    import torch
    import torch.nn as nn

    class StandIn(nn.Module):
        def __init__(self):
            super().__init__()
            self.num_ins, self.num_word, self.entity_dim = num_ins, num_word, entity_dim
            self.word_embedding = nn.Embedding(num_word + 1, word_dim, padding_idx=num_word)
            self.node_encoder = nn.LSTM(word_dim, entity_dim, batch_first=True)
            self.lstm_drop, self.linear_drop = nn.Dropout(0.0), nn.Dropout(linear_dropout)
            self.cq_linear, self.ca_linear = nn.Linear(4 * entity_dim, entity_dim), nn.Linear(entity_dim, 1)
            for i in range(num_ins):
                self.add_module("question_linear%d" % i, nn.Linear(entity_dim, entity_dim))

        def encode_question(self, text):
            out, (h, _) = self.node_encoder(self.lstm_drop(self.word_embedding(text)))
            self.query_hidden_emb, self.query_node_emb = out, h[0][:, None, :]
            self.query_mask = (text != self.num_word).float()

        def init_reason(self, text):
            self.batch_size, self.max_query_word = text.shape
            self.encode_question(text)
            self.relational_ins = torch.zeros(text.shape[0], self.entity_dim, device=text.device)
            self.instructions, self.attn_list = [], []

        def get_instruction(self, relational_ins, step=0, query_node_emb=None):
            node = self.query_node_emb if query_node_emb is None else query_node_emb
            r = relational_ins[:, None, :]
            q = getattr(self, "question_linear%d" % step)(self.linear_drop(node))
            cq = self.cq_linear(self.linear_drop(torch.cat([r, q, q - r, q * r], -1)))
            ca = self.ca_linear(self.linear_drop(cq * self.query_hidden_emb))
            a = torch.softmax(ca + (1 - self.query_mask[:, :, None]) * VERY_NEG, 1)
            return (a * self.query_hidden_emb).sum(1), a

        def forward(self, text, lm=None):
            self.init_reason(text)
            for i in range(self.num_ins):
                self.relational_ins, a = self.get_instruction(self.relational_ins, i)
                self.instructions.append(self.relational_ins)
                self.attn_list.append(a)
            return self.instructions, self.attn_list

    return StandIn().to(device)


def standin_oracle(mod, steps=None, r_in=None):
    """The float64 oracle on what a stand-in (or reference) module holds after an encode."""
    c = lambda t: t.detach().cpu().numpy()      # noqa: E731
    steps = range(mod.num_ins) if steps is None else steps
    B, T, D = mod.query_hidden_emb.shape
    lins = [getattr(mod, "question_linear%d" % s) for s in steps]
    return instructions(c(mod.query_hidden_emb), c(mod.query_node_emb).reshape(B, D), c(mod.query_mask),
                        [c(m.weight) for m in lins], [c(m.bias) for m in lins], c(mod.cq_linear.weight),
                        c(mod.cq_linear.bias), c(mod.ca_linear.weight), c(mod.ca_linear.bias),
                        None if r_in is None else c(r_in))
