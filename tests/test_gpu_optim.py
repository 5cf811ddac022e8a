"""The optimiser step on the GPU (csrc/optim.hip through gnnrag_amd.optim): ``clip_and_step`` / ``step`` of a patched
``torch.optim.Adam`` with ``GNNRAG_HIP_OPTIM=1`` against the float64 oracle (tests/optim_oracle.py) fed the same fp32 inputs.

Bounds.  ``total_norm``: 2e-5 relative (TOL_KERNEL of the project's kernel tests).  p, m, v and the per-step update
``p_after - p_before``, per tensor and step: the largest deviation from the oracle relative to the oracle's largest entry is
at most max(4 x e_torch, 2^-23), e_torch the same figure of torch's own fp32 ``Adam(foreach=False)`` + ``clip_grad_norm_`` on
the CPU (the 4 x rule of tests/test_gpu_bert_encoder.py).  The measured ratios are printed.

Shapes: one element, below / at / above a 16-byte group, below / at / one past / two chunks and one past (4096 elements a
chunk), 2-d tensors, and a parameter that is a view starting one element into its storage (4-byte path)."""
import contextlib
import math
import os
import types
import warnings

import numpy as np
import pytest
import torch

import optim_oracle as oo

pytestmark = pytest.mark.gpu
TOL_KERNEL = 2e-5
FLOOR = 2.0 ** -23
SHAPES = [(1,), (3,), (4,), (255,), (4096,), (4097,), (8193,), (1, 200), (200, 200), (300, 33), (1001,)]
VIEW = 10                                # index of the parameter that starts one element into its storage
MAX_NORM = 1.0


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


@contextlib.contextmanager
def switch(value):
    old = os.environ.get("GNNRAG_HIP_OPTIM")
    if value is None:
        os.environ.pop("GNNRAG_HIP_OPTIM", None)
    else:
        os.environ["GNNRAG_HIP_OPTIM"] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("GNNRAG_HIP_OPTIM", None)
        else:
            os.environ["GNNRAG_HIP_OPTIM"] = old


def _maker(dev, view=VIEW):
    def make_param(i, arr):
        if i != view:
            return torch.tensor(arr, device=dev).requires_grad_()
        base = torch.zeros(arr.size + 1, device=dev)
        base[1:].copy_(torch.from_numpy(arr).reshape(-1))
        p = base[1:].view(arr.shape).requires_grad_()
        assert p.data_ptr() % 16 == 4 and p.is_leaf
        return p
    return make_param


def _hip(case, dev, max_norm=MAX_NORM, view=VIEW, **kw):
    from gnnrag_amd.optim import patch_adam
    with switch("1"):
        snaps, params, opt = oo.run_torch(case, max_norm, device=dev, fused=True, make_param=_maker(dev, view),
                                          patch=patch_adam, **kw)
    assert opt._gnnrag_optim.calls == case["steps"], "the library did not take every step"
    return snaps, params, opt


@pytest.fixture(scope="module")
def ref(dev):
    """The case, the float64 oracle, torch's fp32 CPU run and the library's run of it: computed once, never changed."""
    case = oo.make_case(SHAPES, seed=11)
    assert {g["weight_decay"] for g in case["groups"]} == {0.0, 0.01} and len(case["groups"]) == 2
    want = oo.run_oracle(case, MAX_NORM)
    cpu, _, _ = oo.run_torch(case, MAX_NORM)
    got, params, opt = _hip(case, dev)
    return types.SimpleNamespace(case=case, want=want, cpu=cpu, got=got, params=params, opt=opt)


def _rule(got, cpu, want, start, what):
    """The 4 x rule over every step, part and tensor; returns the worst ratio kernel / bound."""
    worst, lines, bad = 0.0, [], []
    before = [[np.asarray(x, dtype=np.float64) for x in start]] * 3
    for k in range(len(want)):
        parts = {"p": (got[k][0], cpu[k][0], want[k][0]), "m": (got[k][1], cpu[k][1], want[k][1]),
                 "v": (got[k][2], cpu[k][2], want[k][2]),
                 "update": tuple([a - b for a, b in zip(run[k][0], prev)] for run, prev in zip((got, cpu, want), before))}
        for name, (a, b, c) in parts.items():
            for i, (x, y, z) in enumerate(zip(a, b, c)):
                assert (x is None) == (z is None) == (y is None), (what, k, name, i)
                if z is None:
                    continue
                e_k, e_t = oo.rel_dev(x, z), oo.rel_dev(y, z)
                bound = max(4 * e_t, FLOOR)
                lines.append("%s step %d %-6s tensor %2d: kernel %.3e torch %.3e ratio %.3f" % (what, k + 1, name, i, e_k, e_t,
                                                                                              e_k / bound))
                worst = max(worst, e_k / bound)
                if not e_k <= bound:
                    bad.append(lines[-1])
        before = [got[k][0], cpu[k][0], want[k][0]]
    print("\n".join(lines))
    print("%s: worst kernel error / bound = %.3f" % (what, worst))
    assert not bad, "\n".join(bad)
    return worst


def test_total_norm(ref):
    for k in range(3):
        got, want = ref.got[k][3], ref.want[k][3]
        print("step %d: total_norm %.9g, oracle %.9g, relative error %.3e" % (k + 1, got, want, abs(got - want) / want))
        assert abs(got - want) <= TOL_KERNEL * want
        assert (want > MAX_NORM) == (k == 0)


def test_p_m_v_and_the_update_after_every_step(ref):
    _rule(ref.got, ref.cpu, ref.want, ref.case["params"], "adam")
    st = ref.opt.state[ref.params[0]]
    assert st["step"].device.type == "cpu" and st["step"].item() == 3 and st["exp_avg"].is_cuda


def test_a_second_run_gives_the_same_bits(ref, dev):
    again, _, _ = _hip(ref.case, dev)
    for k in range(3):
        assert again[k][3] == ref.got[k][3]
        for a, b in zip(again[k][:3], ref.got[k][:3]):
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes()


def test_the_vector_and_the_element_path_give_the_same_bits(ref, dev):
    """The same case with the last parameter 16-byte aligned instead of one element into its storage."""
    aligned, _, _ = _hip(ref.case, dev, view=-1)
    for k in range(3):
        assert aligned[k][3] == ref.got[k][3]
        for a, b in zip(aligned[k][:3], ref.got[k][:3]):
            assert a[VIEW].tobytes() == b[VIEW].tobytes()


def test_grad_none_keeps_the_bytes_and_gets_no_state(dev):
    case = oo.make_case(SHAPES[:6], seed=5, none_at=((0, 4), (1, 4), (2, 4), (1, 2)))
    got, params, opt = _hip(case, dev, view=-1)
    assert params[4] not in opt.state and got[2][1][4] is None
    assert got[2][0][4].astype(np.float32).tobytes() == case["params"][4].tobytes()
    assert opt.state[params[2]]["step"].item() == 2 and opt.state[params[0]]["step"].item() == 3
    cpu, _, _ = oo.run_torch(case, MAX_NORM)
    _rule(got, cpu, oo.run_oracle(case, MAX_NORM), case["params"], "grad None")


def test_two_hip_steps_then_one_torch_step(ref, dev):
    """State interchange: the switch is flipped between steps."""
    from gnnrag_amd.optim import patch_adam
    case = ref.case
    params, opt = oo.build_torch(case, device=dev, make_param=_maker(dev))
    patch_adam(opt)
    snaps = []
    for k in range(3):
        oo.set_grads(params, case["grads"][k])
        with switch("1" if k < 2 else "0"):
            norm = opt.clip_and_step(params, MAX_NORM)
        snaps.append(oo.snapshot(params, opt, norm))
    assert opt._gnnrag_optim.calls == 2
    _rule(snaps, ref.cpu, ref.want, case["params"], "hip, hip, torch")
    assert abs(snaps[2][3] - ref.want[2][3]) <= TOL_KERNEL * ref.want[2][3]


def test_grad_is_unchanged_by_clip_and_step(ref, dev):
    from gnnrag_amd.optim import patch_adam
    params, opt = oo.build_torch(ref.case, device=dev, make_param=_maker(dev))
    patch_adam(opt)
    oo.set_grads(params, ref.case["grads"][0])                 # norm 3 > max_norm: clip_grad_norm_ would rescale
    with switch("1"):
        opt.clip_and_step(params, MAX_NORM)
    assert opt._gnnrag_optim.calls == 1
    for p, g in zip(params, ref.case["grads"][0]):
        assert p.grad.cpu().numpy().tobytes() == g.tobytes()


def _nan_sets(case, dev, max_norm, view=-1):
    got, _, _ = _hip(case, dev, max_norm=max_norm, view=view)
    cpu, _, _ = oo.run_torch(case, max_norm)
    for k in range(case["steps"]):
        for i, (x, y) in enumerate(zip(got[k][0], cpu[k][0])):
            assert np.array_equal(np.isnan(x), np.isnan(y)), "step %d tensor %d: NaN sets differ" % (k + 1, i)
    return got, cpu


def _plain_groups(n, weight_decay=0.0):
    return [dict(idx=list(range(n)), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay)]


def test_corner_max_norm_far_above_the_norm_equals_step_without_clip(ref, dev):
    from gnnrag_amd.optim import patch_adam
    got, _ = _nan_sets(ref.case, dev, 1e30, view=VIEW)
    params, opt = oo.build_torch(ref.case, device=dev, make_param=_maker(dev))
    patch_adam(opt)
    with switch("1"):
        for k in range(3):
            oo.set_grads(params, ref.case["grads"][k])
            opt.step()
            for x, p in zip(got[k][0], params):
                assert x.astype(np.float32).tobytes() == p.detach().cpu().numpy().tobytes()
    assert opt._gnnrag_optim.calls == 3


def test_corner_one_tensor_of_one_element(dev):
    case = oo.make_case([(1,)], seed=3, groups=_plain_groups(1))
    got, cpu = _nan_sets(case, dev, MAX_NORM)
    _rule(got, cpu, oo.run_oracle(case, MAX_NORM), case["params"], "one element")


def test_corner_all_zero_gradient_leaves_p_bit_for_bit(dev):
    case = oo.make_case(SHAPES[:7], seed=4, steps=1, groups=_plain_groups(7))
    case["grads"][0] = [np.zeros_like(g) for g in case["grads"][0]]
    got, _ = _nan_sets(case, dev, MAX_NORM)
    assert got[0][3] == 0.0
    for x, p in zip(got[0][0], case["params"]):
        assert x.astype(np.float32).tobytes() == p.tobytes()


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_corner_one_inf_or_nan_in_a_gradient(dev, bad):
    case = oo.make_case(SHAPES[:7], seed=6, steps=2, groups=_plain_groups(7))
    case["grads"][0][5][4096] = bad                               # the second chunk of the 4097-element tensor
    got, cpu = _nan_sets(case, dev, MAX_NORM)
    n_nan = sum(int(np.isnan(x).sum()) for x in got[0][0])
    if math.isinf(bad):
        assert math.isinf(got[0][3]) and n_nan == 1                 # coefficient 0: inf * 0 in that one entry
    else:
        assert math.isnan(got[0][3]) and n_nan == sum(x.size for x in got[0][0])


def test_scheduler_and_hooks_on_the_library_path(ref, dev):
    from gnnrag_amd.optim import patch_adam
    params, opt = oo.build_torch(ref.case, device=dev, make_param=_maker(dev))
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, 0.5)
    patch_adam(opt)
    seen = {"pre": 0, "post": 0}
    opt.register_step_pre_hook(lambda o, a, k: seen.__setitem__("pre", seen["pre"] + 1))
    opt.register_step_post_hook(lambda o, a, k: seen.__setitem__("post", seen["post"] + 1))
    with switch("1"), warnings.catch_warnings():
        warnings.simplefilter("error")
        for k in range(2):
            oo.set_grads(params, ref.case["grads"][k])
            if k == 0:
                opt.clip_and_step(params, MAX_NORM)
            else:
                opt.step()
            sched.step()
            assert seen == {"pre": k + 1, "post": k + 1}
    assert opt._gnnrag_optim.calls == 2 and opt.param_groups[0]["lr"] == pytest.approx(0.25e-3)


# -- the trainer's loop ----------------------------------------------------------------------------------------------------

class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.emb = torch.nn.Embedding(40, 12)
        self.l1 = torch.nn.Linear(12, 20)
        self.l2 = torch.nn.Linear(20, 1)
        self.frozen = torch.nn.Parameter(torch.ones(3), requires_grad=False)      # in named_parameters, never has a grad

    def forward(self, batch, training=False):
        ids, target = batch
        out = self.l2(torch.tanh(self.l1(self.emb(ids)))).squeeze(-1)
        loss = ((out - target) ** 2).mean() * 50.0
        return loss, None, None, ([1.0] * len(ids), [0.5] * len(ids))


class _Data:
    num_data = 12

    def __init__(self, device, dtype):
        rng = np.random.default_rng(2)
        self.ids = torch.from_numpy(rng.permutation(40)[:12].reshape(3, 4)).to(device)      # distinct rows of the table
        self.target = torch.from_numpy(rng.standard_normal((3, 4))).to(device=device, dtype=dtype)
        self.resets = 0

    def reset_batches(self, is_sequential=True):
        self.resets += 1

    def get_batch(self, iteration, batch_size, fact_drop):
        return self.ids[iteration], self.target[iteration]


def _trainer(device, dtype, state):
    model = _Tiny().to(device=device, dtype=dtype)
    model.load_state_dict({k: v.to(device=device, dtype=dtype) for k, v in state.items()})
    opt = torch.optim.Adam(filter(lambda p: p.requires_grad, model.parameters()), lr=1e-3)
    return types.SimpleNamespace(model=model, optim_model=opt, train_data=_Data(device, dtype),
                                 args={"batch_size": 4, "fact_drop": 0, "gradient_clip": 1.0})


def _plain_epoch(tr):
    tr.model.train()
    losses = []
    for it in range(3):
        batch = tr.train_data.get_batch(it, 4, 0)
        tr.optim_model.zero_grad()
        loss = tr.model(batch, training=True)[0]
        loss.backward()
        torch.nn.utils.clip_grad_norm_([p for _, p in tr.model.named_parameters()], 1.0)
        tr.optim_model.step()
        losses.append(loss.item())
    return losses


def test_a_tiny_model_through_patch_trainers_epoch(dev):
    from gnnrag_amd import install
    torch.manual_seed(0)
    state = {k: v.clone() for k, v in _Tiny().state_dict().items()}
    oracle = _trainer("cpu", torch.float64, state)
    want_losses = _plain_epoch(oracle)
    plain = _trainer(dev, torch.float32, state)
    plain_losses = _plain_epoch(plain)
    tr = _trainer(dev, torch.float32, state)
    optimizer = tr.optim_model
    assert install.patch_trainer(tr) is tr and install.patch_trainer(tr) is tr and tr.optim_model is optimizer
    with switch("1"):
        loss, extras, h1, f1 = tr.train_epoch()
    assert optimizer._gnnrag_optim.calls == 3 and tr.train_data.resets == 1 and tr.model.training
    assert extras == [0, 0] and h1 == [1.0] * 12 and f1 == [0.5] * 12
    assert abs(loss - np.mean(want_losses)) <= 1e-5 * abs(np.mean(want_losses))
    assert abs(np.mean(plain_losses) - np.mean(want_losses)) <= 1e-5 * abs(np.mean(want_losses))
    for (name, w), g, t in zip(oracle.model.named_parameters(), tr.model.parameters(), plain.model.parameters()):
        z = w.detach().numpy()
        e_k, e_t = oo.rel_dev(g.detach().cpu().double().numpy(), z), oo.rel_dev(t.detach().cpu().double().numpy(), z)
        print("%-10s kernel %.3e torch %.3e ratio %.3f" % (name, e_k, e_t, e_k / max(4 * e_t, FLOOR)))
        assert e_k <= max(4 * e_t, FLOOR), name
    assert set(optimizer.state_dict()["state"]) == set(plain.optim_model.state_dict()["state"])
