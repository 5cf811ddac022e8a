"""Float64 restatement of the optimiser step of a training step: ``torch.nn.utils.clip_grad_norm_`` over a list of gradients
followed by ``torch.optim.Adam.step`` (``_single_tensor_adam``, non-capturable: no amsgrad, no maximize, coupled weight
decay) over a list of tensors in parameter groups - per-tensor step counts, ``weight_decay``, gradients that are ``None``.
Plain numpy, written from the formulas; tests/test_optim_host.py holds it against torch in float64.

Also the shared case generator and the torch runner of the optimiser tests (host and GPU)."""
import math

import numpy as np
import torch

CLIP_EPS = 1e-6                     # clip_grad_norm_: max_norm / (total_norm + 1e-6)


class AdamOracle:
    """params: arrays (copied to float64); groups: dicts with ``idx`` (the parameters of the group), ``lr``, ``betas``,
    ``eps``, ``weight_decay``.  ``lr`` of a group may be changed between steps (a scheduler)."""

    def __init__(self, params, groups):
        self.p = [np.array(x, dtype=np.float64) for x in params]
        self.groups = [dict(g) for g in groups]
        self.state = {}             # index -> {"step", "m", "v"}; absent until the parameter first has a gradient

    @staticmethod
    def total_norm(grads):
        return math.sqrt(sum(float((np.asarray(g, dtype=np.float64) ** 2).sum()) for g in grads if g is not None))

    @classmethod
    def clip(cls, grads, max_norm):
        """(total_norm, coefficient, the gradients as clip_grad_norm_ leaves them)."""
        total = cls.total_norm(grads)
        coef = max_norm / (total + CLIP_EPS)
        if coef == coef:
            coef = min(coef, 1.0)
        with np.errstate(invalid="ignore"):
            return total, coef, [None if g is None else np.asarray(g, dtype=np.float64) * coef for g in grads]

    def step(self, grads, max_norm=None):
        """One step; grads[i] is None for a parameter without gradient.  Returns the total norm (None without clipping)."""
        total = None
        if max_norm is not None:
            total, _, grads = self.clip(grads, max_norm)
        for grp in self.groups:
            beta1, beta2 = grp["betas"]
            for i in grp["idx"]:
                if grads[i] is None:
                    continue
                st = self.state.setdefault(i, {"step": 0, "m": np.zeros_like(self.p[i]), "v": np.zeros_like(self.p[i])})
                st["step"] += 1
                g = np.asarray(grads[i], dtype=np.float64)
                with np.errstate(invalid="ignore", over="ignore"):
                    if grp["weight_decay"] != 0:
                        g = g + grp["weight_decay"] * self.p[i]
                    st["m"] = st["m"] + (g - st["m"]) * (1 - beta1)
                    st["v"] = st["v"] * beta2 + (1 - beta2) * g * g
                    step_size = grp["lr"] / (1 - beta1 ** st["step"])
                    denom = np.sqrt(st["v"]) / math.sqrt(1 - beta2 ** st["step"]) + grp["eps"]
                    self.p[i] = self.p[i] - step_size * st["m"] / denom
        return total


# -- cases -----------------------------------------------------------------------------------------------------------------

def make_case(shapes, steps=3, seed=0, norms=(3.0, 0.4, 0.7), groups=None, none_at=()):
    """fp32 parameters and per-step gradients of the given shapes; the gradients of step k are scaled to a total norm of
    norms[k].  none_at: (step, index) pairs whose gradient is None.  groups default to two halves with different lr and
    weight_decay 0 / 0.01."""
    rng = np.random.default_rng(seed)
    params = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    grads = []
    for k in range(steps):
        gs = [None if (k, i) in none_at else rng.standard_normal(s).astype(np.float32) for i, s in enumerate(shapes)]
        total = AdamOracle.total_norm(gs)
        gs = [None if g is None else (g * (norms[k] / total)).astype(np.float32) for g in gs]
        grads.append(gs)
    if groups is None:
        half = (len(shapes) + 1) // 2
        groups = [dict(idx=list(range(half)), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
                  dict(idx=list(range(half, len(shapes))), lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)]
        groups = [g for g in groups if g["idx"]]
    return {"params": params, "grads": grads, "groups": groups, "steps": steps}


def run_oracle(case, max_norm, gamma_after=None, dtype=np.float64):
    """Snapshots [(p list, m list, v list, norm)] after every step; gamma_after: {step: gamma} multiplies every lr after
    that step (ExponentialLR)."""
    o = AdamOracle(case["params"], case["groups"])
    snaps = []
    for k in range(case["steps"]):
        norm = o.step(case["grads"][k], max_norm)
        n = len(o.p)
        snaps.append(([x.copy() for x in o.p],
                      [o.state[i]["m"].copy() if i in o.state else None for i in range(n)],
                      [o.state[i]["v"].copy() if i in o.state else None for i in range(n)], norm))
        if gamma_after and k in gamma_after:
            for g in o.groups:
                g["lr"] = g["lr"] * gamma_after[k]
    return snaps


def build_torch(case, dtype=torch.float32, device="cpu", make_param=None):
    """(params, optimizer) as torch builds them: ``Adam(foreach=False)`` over the case's groups."""
    if make_param is None:
        def make_param(i, arr):
            return torch.tensor(arr, dtype=dtype, device=device).requires_grad_()
    params = [make_param(i, a) for i, a in enumerate(case["params"])]
    groups = [dict(params=[params[i] for i in g["idx"]], lr=g["lr"], betas=g["betas"], eps=g["eps"],
                   weight_decay=g["weight_decay"]) for g in case["groups"]]
    return params, torch.optim.Adam(groups, foreach=False)


def set_grads(params, grads, dtype=torch.float32):
    for p, g in zip(params, grads):
        p.grad = None if g is None else torch.tensor(g, dtype=dtype, device=p.device).reshape(p.shape)


def snapshot(params, opt, norm):
    def np64(t):
        return None if t is None else t.detach().cpu().double().numpy().copy()
    st = [opt.state.get(p) or {} for p in params]
    return ([np64(p) for p in params], [np64(s.get("exp_avg")) for s in st], [np64(s.get("exp_avg_sq")) for s in st],
            None if norm is None else float(norm))


def run_torch(case, max_norm, dtype=torch.float32, device="cpu", fused=False, gamma_after=None, make_param=None,
              patch=None):
    """The same steps through torch.  fused=False: ``clip_grad_norm_`` + ``optimizer.step()``; fused=True:
    ``optimizer.clip_and_step`` of an optimiser patched by ``patch`` (gnnrag_amd.optim.patch_adam).  Returns
    (snapshots, params, optimizer)."""
    params, opt = build_torch(case, dtype, device, make_param)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=1.0) if gamma_after else None
    if patch is not None:
        patch(opt)
    snaps = []
    for k in range(case["steps"]):
        set_grads(params, case["grads"][k], dtype)
        if fused:
            norm = opt.clip_and_step(params, max_norm)
        else:
            norm = torch.nn.utils.clip_grad_norm_(params, max_norm)
            opt.step()
        snaps.append(snapshot(params, opt, norm))
        if gamma_after and k in gamma_after:
            sched.gamma = gamma_after[k]
            sched.step()
    return snaps, params, opt


def rel_dev(got, want):
    """Largest deviation relative to the largest entry of ``want`` (float64 arrays)."""
    scale = max(float(np.abs(want).max()), 1e-300)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max()) / scale
