"""Float64 numpy restatement of the instruction update between two ReaRev iterations (rearev.py:217-221 ->
query_update.py:26-44 with Fusion :6-16) and of its backward, shared by tests/test_query_reform_train_host.py and
tests/test_gpu_query_reform_train*.py.  For reform j < n and question b:

    x = q_j[b]      y = sum_n seed[b,n] E[b,n,:]      f = [x, y, x - y]
    a_r = W_r^j f   a_g = W_g^j f   g = sigmoid(a_g)  out = g a_r + (1 - g) x

    da_r = G g      da_g = G (a_r - x) g (1 - g)      df = W_r^T da_r + W_g^T da_g
    dx = G (1 - g) + df[0:D] + df[2D:3D]              dy = df[D:2D] - df[2D:3D]
    dW_r = sum_b da_r[b] (x) f[b]   dW_g alike        d_ent[b,n,:] = seed[b,n] sum_j dy_j[b]

A reform whose upstream gradient is None was not used: its dq / dW are None and it adds nothing to d_ent."""
import numpy as np


def _f(a):
    return np.asarray(a, dtype=np.float64)


def forward(qs, seed, ent, W_rs, W_gs):
    """(out [n,B,D], saved) in float64; ``saved`` is what :func:`backward` reads."""
    seed, ent = _f(seed), _f(ent)
    D = _f(qs[0]).shape[1]
    y = np.einsum("bn,bnd->bd", seed, ent[:, :, :D])
    outs, per = [], []
    for q, W_r, W_g in zip(qs, W_rs, W_gs):
        x, W_r, W_g = _f(q), _f(W_r), _f(W_g)
        f = np.concatenate([x, y, x - y], axis=1)
        a_r, a_g = f @ W_r.T, f @ W_g.T
        g = 1.0 / (1.0 + np.exp(-a_g))
        outs.append(g * a_r + (1.0 - g) * x)
        per.append(dict(x=x, f=f, a_r=a_r, g=g, W_r=W_r, W_g=W_g))
    return np.stack(outs), dict(seed=seed, per=per, N=ent.shape[1])


def backward(saved, g_outs):
    """The gradients of ``sum_j sum(out_j * g_outs[j])`` (a None entry: that reform is unused) as a dict: dq / dW_r / dW_g
    lists per reform (None for an unused one), d_ent [B,N,D]."""
    seed, per = saved["seed"], saved["per"]
    B, D = per[0]["x"].shape
    dq, dW_r, dW_g, dy_sum = [], [], [], np.zeros((B, D))
    for p, G in zip(per, g_outs):
        if G is None:
            dq.append(None), dW_r.append(None), dW_g.append(None)
            continue
        G, g = _f(G), p["g"]
        da_r = G * g
        da_g = G * (p["a_r"] - p["x"]) * g * (1.0 - g)
        df = da_r @ p["W_r"] + da_g @ p["W_g"]
        dq.append(G * (1.0 - g) + df[:, :D] + df[:, 2 * D:])
        dy_sum = dy_sum + (df[:, D:2 * D] - df[:, 2 * D:])
        dW_r.append(da_r.T @ p["f"])
        dW_g.append(da_g.T @ p["f"])
    return dict(dq=dq, dW_r=dW_r, dW_g=dW_g, d_ent=seed[:, :, None] * dy_sum[:, None, :])


def seeds(B, N, rng):
    """seed_info [B,N] fp32 of the test cases: question 0 has two seeds where N allows, one of weight 0.5 and one in slot
    N - 1; the last question of a batch of more than one has no seed; the others have one seed."""
    s = np.zeros((B, N), dtype=np.float32)
    for b in range(B):
        if b == B - 1 and B > 1:
            continue
        if b == 0:
            s[b, N - 1] = 1.0
            if N > 1:
                s[b, int(rng.integers(0, N - 1))] = 0.5
        else:
            s[b, int(rng.integers(0, N))] = 1.0
    return s


def train_case(B, N, D, n, seed=0, ld=None):
    """A random case in fp32: qs / W_rs / W_gs lists of n, seed [B,N] (see :func:`seeds`), ent [B,N,ld or D], G [n,B,D]."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, dtype=np.float32)      # noqa: E731
    k = 1.0 / np.sqrt(3.0 * D)
    return dict(qs=[f32(np.tanh(rng.standard_normal((B, D)))) for _ in range(n)],
                W_rs=[f32(rng.uniform(-k, k, (D, 3 * D))) for _ in range(n)],
                W_gs=[f32(rng.uniform(-k, k, (D, 3 * D))) for _ in range(n)],
                seed=seeds(B, N, rng), ent=f32(rng.standard_normal((B, N, D if ld is None else ld))),
                G=f32(rng.standard_normal((n, B, D))))


def standin(D, n):
    """The part of ReaRev that rearev.py:217-221 runs, on this package's ``QueryReform``: ``reform{j}`` modules and
    ``instruction.instructions`` (a list of [B,1,D] tensors); ``loop`` is those lines, one round per node state given."""
    import torch
    from gnnrag_amd.modules.query_update import QueryReform

    class Instr(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.instructions = []

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.num_ins = n
            self.instruction = Instr()
            for j in range(n):
                self.add_module("reform" + str(j), QueryReform(D))

        def loop(self, ins0, ents, seed, mask):
            self.instruction.instructions = [t.unsqueeze(1) for t in ins0]
            for ent in ents:
                for j in range(self.num_ins):
                    reform = getattr(self, "reform" + str(j))
                    q = reform(self.instruction.instructions[j].squeeze(1), ent, seed, mask)
                    self.instruction.instructions[j] = q.unsqueeze(1)
            return [t.squeeze(1) for t in self.instruction.instructions]

    return Model()
