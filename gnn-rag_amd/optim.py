"""The optimiser step of a training step on the MI355X (csrc/optim.hip).

``Trainer_KBQA.train_epoch`` ends every step with ``torch.nn.utils.clip_grad_norm_`` over the model's parameters and
``torch.optim.Adam.step`` (``train_model.py:228-230``): in torch a few dozen multi-tensor launches over ~60 small tensors and
two or three embedding tables.  ``patch_adam(optimizer)`` patches an EXISTING ``torch.optim.Adam`` in place - the object
stays the same and stays an instance of its class, so a scheduler that holds it keeps working - and gives it

* ``optimizer.clip_and_step(clip_params, max_norm) -> total_norm``: both statements as three launches
  (``gnnrag_grad_norm`` + ``gnnrag_adam_step``), ``total_norm`` a 0-dim device tensor as ``clip_grad_norm_`` returns it;
* ``optimizer.step()``: the Adam step as one launch.

NOTE: the fused call does NOT rescale ``.grad``.  ``clip_grad_norm_`` multiplies every gradient by the clip coefficient in
place; here the coefficient is applied as the gradients are read and ``.grad`` keeps the values ``backward`` left (the
trainer clears them at the top of the next step).

Both take the library only with ``GNNRAG_HIP_OPTIM=1`` (read at every call, default off) and when, at that call,

* every parameter with a gradient is a CUDA fp32 dense contiguous tensor on one device, and so is its gradient and (where
  it exists) its state; ``step`` is torch's per-parameter CPU scalar;
* no group asks for ``amsgrad``, ``maximize``, ``capturable``, ``differentiable``, ``decoupled_weight_decay`` or ``fused``;
  ``lr`` and the betas are Python numbers; no ``closure``, no gradient scaler attached;
* for ``clip_and_step``: ``max_norm > 0`` and the parameters of ``clip_params`` that have a gradient are exactly the
  optimiser's parameters that have one (the trainer's case: one table serves both calls).  Otherwise torch's own
  ``clip_grad_norm_`` runs (and rescales ``.grad``), followed by ``step()`` under its own rules.

Anything else runs what was there before, unchanged.  The state is torch's own: ``exp_avg`` / ``exp_avg_sq`` are created as
``Adam._init_group`` creates them, ``step`` is the same CPU scalar tensor incremented by the same float addition (made on the
tensor's own memory through a numpy view: a dispatched ``step += 1`` costs ~4 us per parameter), a parameter whose grad is
``None`` is skipped and gets no state - ``state_dict()`` is interchangeable and the switch can be flipped between steps.
Step pre / post hooks run once per step, and ``LRScheduler`` sees the step (no "before optimizer.step()" warning).

The segment table (``gnnrag_optim_seg``, 80 bytes per tensor) is kept on the host, copied into one of two pinned buffers
and uploaded with one non-blocking copy per step; a pinned buffer is rewritten only after the event behind its last upload.
Pointers and sizes are rewritten only when a tensor moved; the scalars (``lr / (1 - beta1^t)``, ``sqrt(1 - beta2^t)``, ...)
are formed in double as torch forms them, every step.
"""
from __future__ import annotations

import os
import types

import numpy as np
import torch
from torch.optim.optimizer import Optimizer

from . import ops

DEFAULT = "0"        # GNNRAG_HIP_OPTIM when unset (the rule for a later flip)
_SCALARS = ("beta1", "beta2", "om_beta1", "om_beta2", "eps", "weight_decay", "step_size", "bc2_sqrt")
_BARRED = ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay", "fused")


def enabled() -> bool:
    """Whether a patched optimiser uses the library (read at every call: the switch can change between steps)."""
    return os.environ.get("GNNRAG_HIP_OPTIM", DEFAULT) == "1"


def _scalar_dtype():
    try:
        from torch.optim.optimizer import _get_scalar_dtype
        return _get_scalar_dtype()
    except ImportError:                      # older torch: the step count is a float32 scalar
        return torch.float32


def _number(x) -> bool:
    return isinstance(x, (int, float)) and not isinstance(x, bool)


def _f32_dense(t, device) -> bool:
    return (t.dtype == torch.float32 and t.layout == torch.strided and t.device == device and t.is_contiguous())


class _Upload:
    __slots__ = ("pinned", "host", "dev", "event")


class _State:
    """What a patched optimiser keeps between steps: the host table, two pinned copies with their events, two device tables."""

    def __init__(self, prev_step):
        self.prev_step = prev_step           # optimizer.step as it was (a scheduler's wrapper, or the class's own)
        self.master = np.zeros(0, dtype=ops.OPTIM_SEG_DTYPE)
        self.ptr_key = None                  # (pointers, sizes) the master holds
        self.n_chunks = 0
        self.uploads = []
        self.flip = 0
        self.pending = None                  # (entries, clip coefficient) of the step in flight
        self.step_views = {}                 # id(step tensor) -> (the tensor, its numpy view)
        self.checked = {}                    # id(parameter) -> (parameter, step, exp_avg, exp_avg_sq, device) found eligible
        self.calls = 0                       # steps taken on the library

    def upload(self, T: int, device) -> torch.Tensor:
        """The first T entries of the master as a device table (uint8), uploaded on the current stream."""
        if not self.uploads or self.uploads[0].host.shape[0] < T or self.uploads[0].dev.device != device:
            cap = max(64, 2 * T)
            self.uploads = []
            for _ in range(2):
                u = _Upload()
                u.pinned = torch.empty(cap * ops.OPTIM_SEG_BYTES, dtype=torch.uint8, pin_memory=True)
                u.host = u.pinned.numpy().view(ops.OPTIM_SEG_DTYPE)
                u.dev = ops._buf((cap * ops.OPTIM_SEG_BYTES,), torch.uint8, device, "optim: segment table")
                u.event = torch.cuda.Event()
                self.uploads.append(u)
        u = self.uploads[self.flip]
        self.flip ^= 1
        u.event.synchronize()                # the upload that last read this pinned buffer (two steps ago) is done
        u.host[:T] = self.master[:T]
        nbytes = T * ops.OPTIM_SEG_BYTES
        u.dev[:nbytes].copy_(u.pinned[:nbytes], non_blocking=True)
        u.event.record()
        return u.dev


def _entries(opt):
    """[(p, grad, group)] of every parameter with a gradient, in group order, when the step can run on the library at this
    call; else None."""
    if getattr(opt, "grad_scale", None) is not None or getattr(opt, "found_inf", None) is not None:
        return None
    out, device, checked = [], None, opt._gnnrag_optim.checked
    for group in opt.param_groups:
        if any(group.get(k) for k in _BARRED):
            return None
        betas = group["betas"]
        if not (_number(group["lr"]) and _number(betas[0]) and _number(betas[1]) and _number(group["eps"]) and
                _number(group["weight_decay"])):
            return None
        for p in group["params"]:
            g = p.grad
            if g is None:
                continue
            if device is None:
                device = p.device
                if device.type != "cuda":
                    return None
            if not (_f32_dense(p, device) and _f32_dense(g, device) and g.shape == p.shape):
                return None
            st = opt.state.get(p)
            if st:
                step, m, v = st.get("step"), st.get("exp_avg"), st.get("exp_avg_sq")
                seen = checked.get(id(p))
                # the state tensors are checked once: the same objects next step are the same kind of tensor
                if not (seen is not None and seen[0] is p and seen[1] is step and seen[2] is m and seen[3] is v and
                        seen[4] == device):
                    if not (isinstance(step, torch.Tensor) and step.device.type == "cpu" and step.numel() == 1 and
                            not step.requires_grad):
                        return None
                    if not (isinstance(m, torch.Tensor) and isinstance(v, torch.Tensor) and _f32_dense(m, device) and
                            _f32_dense(v, device) and m.shape == p.shape and v.shape == p.shape):
                        return None
                    checked[id(p)] = (p, step, m, v, device)
            out.append((p, g, group))
    if not out or not any(p.numel() for p, _, _ in out):
        return None
    return out


def _same_set(entries, clip_params) -> bool:
    if isinstance(clip_params, torch.Tensor):
        clip_params = [clip_params]
    with_grad = [p for p in clip_params if p.grad is not None]
    return len(with_grad) == len(entries) and {id(p) for p in with_grad} == {id(p) for p, _, _ in entries}


def _fill_table(st: _State, opt, entries):
    """Torch's bookkeeping of a step (lazy state, ``step += 1``) and the host table of it.  Returns (T, n_chunks)."""
    rows, scal, cache = [], [], {}
    for p, g, group in entries:
        state = opt.state[p]
        if len(state) == 0:                                     # Adam._init_group
            state["step"] = torch.tensor(0.0, dtype=_scalar_dtype())
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        step_t = state["step"]
        view = st.step_views.get(id(step_t))
        if view is None or view[0] is not step_t:
            if len(st.step_views) > 8192:                       # tensors of states long replaced
                st.step_views.clear()
            view = st.step_views[id(step_t)] = (step_t, step_t.numpy())
        # torch's ``step_t += 1`` on the tensor's own memory (a CPU scalar): the same float addition without the ~4 us
        # of a dispatched torch op per parameter
        np.add(view[1], 1, out=view[1])
        if p.numel() == 0:
            continue
        key = (id(group), float(view[1]))
        s = cache.get(key)
        if s is None:                                           # _single_tensor_adam, in double like Python
            beta1, beta2 = group["betas"]
            step = key[1]
            bias_correction1 = 1 - beta1 ** step
            bias_correction2 = 1 - beta2 ** step
            s = cache[key] = (beta1, beta2, 1 - beta1, 1 - beta2, group["eps"], group["weight_decay"],
                              group["lr"] / bias_correction1, bias_correction2 ** 0.5)
        scal.append(s)
        rows.append((p.data_ptr(), g.data_ptr(), state["exp_avg"].data_ptr(), state["exp_avg_sq"].data_ptr(), p.numel()))
    T = len(rows)
    ptr_key = tuple(rows)
    if st.master.shape[0] < T:
        st.master = np.zeros(max(64, 2 * T), dtype=ops.OPTIM_SEG_DTYPE)
        st.ptr_key = None
    tab = st.master[:T]
    if st.ptr_key != ptr_key:                                   # something moved (or the first step): pointers and sizes
        cols = list(zip(*rows))
        for name, col in zip(("p", "g", "m", "v"), cols):
            tab[name] = np.array(col, dtype=np.uint64)
        tab["n"] = cols[4]
        first, st.n_chunks = ops.optim_chunks(cols[4])
        tab["first_chunk"] = first
        st.ptr_key = ptr_key
    for name, col in zip(_SCALARS, zip(*scal)):
        tab[name] = col
    return T, st.n_chunks


def _hip_step(self, closure=None):
    """The body of the step on the library; runs inside ``Optimizer.profile_hook_step`` (hooks, profiler range)."""
    st = self._gnnrag_optim
    entries, clip = st.pending
    st.pending = None
    with torch.no_grad():
        T, n_chunks = _fill_table(st, self, entries)
        device = entries[0][0].device
        with torch.cuda.device(device):
            table = st.upload(T, device)
        total = None
        if clip is not None:
            out2 = ops.grad_norm(table, T, n_chunks, clip)
            ops.adam_step(table, T, n_chunks, out2[1:])
            total = out2[0]
        else:
            ops.adam_step(table, T, n_chunks, None)
    st.calls += 1
    return total


_hip_step_hooked = Optimizer.profile_hook_step(_hip_step)


def _run_hip(opt, entries, clip):
    opt._gnnrag_optim.pending = (entries, clip)
    opt._opt_called = True                   # what LRScheduler's wrapper of step() records
    if hasattr(opt, "_step_count"):          # older torch: the scheduler counts the calls of its wrapper
        opt._step_count += 1
    return _hip_step_hooked(opt)


def _step(self, closure=None):
    """``optimizer.step`` of a patched optimiser."""
    entries = _entries(self) if (closure is None and enabled()) else None
    if entries is None:
        self._opt_called = True
        prev = self._gnnrag_optim.prev_step
        return prev() if closure is None else prev(closure)
    _run_hip(self, entries, None)
    return None


# LRScheduler looks for this mark on ``optimizer.step``: without it, it wraps the step (when created after the patch) or
# warns that the step was overridden (when created before).  What its wrapper does - set ``_opt_called`` - _step does.
_step._wrapped_by_lr_sched = True


def _clip_and_step(self, clip_params, max_norm):
    """``clip_grad_norm_(clip_params, max_norm)`` followed by ``step()``; returns the total norm (a 0-dim tensor).  On the
    library path (see the module docstring) ``.grad`` is NOT rescaled: the clip coefficient is applied as the gradients are
    read."""
    if isinstance(clip_params, torch.Tensor):
        clip_params = [clip_params]
    else:
        clip_params = list(clip_params)
    entries = None
    if enabled() and _number(max_norm) and max_norm > 0:
        entries = _entries(self)
        if entries is not None and not _same_set(entries, clip_params):
            entries = None
    if entries is None:
        total = torch.nn.utils.clip_grad_norm_(clip_params, max_norm)
        self.step()
        return total
    return _run_hip(self, entries, float(max_norm))


def _train_epoch(trainer):
    """One epoch as ``Trainer_KBQA.train_epoch`` runs it (``train_model.py:209-233``; the same walk
    ``tools/time_train_step.py`` times): shuffled batches, ``zero_grad`` -> forward -> ``backward`` -> clip + Adam ->
    ``loss.item()``, with the clip and the Adam step (``:228-230``) as ONE ``clip_and_step`` call.  Returns what the
    reference's method returns: (mean loss, [0, 0], the H@1 of every question, the F1 of every question)."""
    import math
    args, data, model, optimizer = trainer.args, trainer.train_data, trainer.model, trainer.optim_model
    model.train()
    data.reset_batches(is_sequential=False)
    steps = range(math.ceil(data.num_data / args["batch_size"]))
    try:
        from tqdm import tqdm                                   # the reference's progress bar, where it is installed
        steps = tqdm(steps)
    except ImportError:
        pass
    losses, h1_all, f1_all = [], [], []
    for it in steps:
        batch = data.get_batch(it, args["batch_size"], args["fact_drop"])
        optimizer.zero_grad()
        loss, _, _, tp_list = model(batch, training=True)
        h1, f1 = tp_list
        h1_all.extend(h1)
        f1_all.extend(f1)
        loss.backward()
        optimizer.clip_and_step([p for _, p in model.named_parameters()], args["gradient_clip"])
        losses.append(loss.item())
    return np.mean(losses), [0, 0], h1_all, f1_all


def patch_trainer(trainer):
    """``patch_adam(trainer.optim_model)`` and ``trainer.train_epoch`` bound to :func:`_train_epoch` on the instance (the
    reference's file is untouched).  Idempotent; returns the trainer."""
    patch_adam(trainer.optim_model)
    if not getattr(trainer, "_gnnrag_train_epoch_patched", False):
        trainer.train_epoch = types.MethodType(_train_epoch, trainer)
        trainer._gnnrag_train_epoch_patched = True
    return trainer


def patch_adam(optimizer):
    """Patches a ``torch.optim.Adam`` instance in place (see the module docstring): adds ``clip_and_step`` and routes
    ``step()`` through the library when the call is eligible.  Idempotent; returns the optimiser."""
    if not isinstance(optimizer, torch.optim.Adam):
        raise TypeError("patch_adam: expected a torch.optim.Adam, got %s" % type(optimizer).__name__)
    if getattr(optimizer, "_gnnrag_optim", None) is not None:
        return optimizer
    optimizer._gnnrag_optim = _State(optimizer.step)
    # bound methods: LRScheduler wraps ``optimizer.step.__func__`` when it is created after this
    optimizer.step = types.MethodType(_step, optimizer)
    optimizer.clip_and_step = types.MethodType(_clip_and_step, optimizer)
    return optimizer
