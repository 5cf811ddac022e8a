"""Guarded buffers for tests: every tensor handed out is an exact-sized view in the middle of a larger uint8 block,
with a guard of known bytes directly in front of it and directly behind it (no rounding: the back guard starts at the
first byte after the view).  ``check()`` finds a write outside a view, the body fills (0x00, 0xFF, or the bytes a previous
call left in the buffer of the same role) find a result that depends on what a buffer held before the call.

Device-agnostic on purpose (tests/test_guarded_harness.py proves the harness itself on CPU tensors); the GPU tests
install ``Guard.buf`` in place of ``gnnrag_amd.ops._buf``, the one function through which the binding allocates what it
hands to the library.

Guard bytes:
  * float buffers (allocated or wrapped): 0xFF, i.e. NaN - a read past the end that reaches a result shows;
  * integer / raw byte buffers allocated here (workspaces, structure memory, index outputs): the int32 value 1 repeated
    (01 00 00 00) - not zero, so a memset or a zero row that overruns is seen, and a valid index, so that a stray read
    which is then used as an index stays inside memory the test owns;
  * wrapped integer inputs: zero bytes (a valid index, for the same reason)."""
import math

import torch

GUARD_BYTES = 64 * 1024          # each side; a multiple of 512: the view keeps the allocator's 512-byte alignment
FILL_ZERO, FILL_ONES, FILL_LEFTOVERS = 0x00, 0xFF, "leftovers"
_PAT_NAN, _PAT_ONE, _PAT_ZERO = (0xFF,) * 4, (1, 0, 0, 0), (0,) * 4


class GuardError(AssertionError):
    pass


class _Block:
    __slots__ = ("role", "raw", "nbytes", "pattern", "view", "copy")


def _nbytes(shape, dtype):
    shape = (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)
    return shape, math.prod(shape) * torch.empty(0, dtype=dtype).element_size()


class Guard:
    def __init__(self, device, guard_bytes: int = GUARD_BYTES, fill=FILL_ZERO):
        assert guard_bytes >= 512 and guard_bytes % 512 == 0
        self.device, self.G, self.fill = torch.device(device), int(guard_bytes), fill
        self.blocks = []
        self._last = {}          # (role, nbytes) -> the block of that role allocated before the current one
        self._expected = {}
        self.leftover_hits = 0
        self.sizes = {}          # role -> bytes of the last buffer asked for under that name
        self.short = {}          # role -> bytes to hold back: the caller sees (and states) a buffer that much smaller

    # -- allocation ---------------------------------------------------------------------------------------------
    def _expect(self, device, pattern):
        key = (str(device), pattern)
        if key not in self._expected:
            self._expected[key] = torch.tensor(pattern, dtype=torch.uint8, device=device).repeat(self.G // 4)
        return self._expected[key]

    def _block(self, shape, dtype, device, role, pattern):
        shape, n = _nbytes(shape, dtype)
        G = self.G
        b = _Block()
        b.role, b.nbytes, b.pattern, b.copy = role, n, pattern, None
        b.raw = torch.empty(2 * G + n, dtype=torch.uint8, device=device)
        exp = self._expect(b.raw.device, pattern)
        b.raw[:G].copy_(exp[:G])
        b.raw[G + n:].copy_(exp[:G])              # the pattern restarts at the first byte after the view
        b.view = b.raw[G: G + n].view(dtype).view(shape)
        self.blocks.append(b)
        return b

    def alloc(self, shape, dtype, device=None, fill=None, role="buffer"):
        """An uninitialised buffer as the library sees one: the body holds ``fill`` bytes (default: this guard's current
        fill; FILL_LEFTOVERS = a byte copy of the previous buffer of the same role and size, 0xFF when there is none)."""
        device = self.device if device is None else device
        fill = self.fill if fill is None else fill
        b = self._block(shape, dtype, device, role, _PAT_NAN if dtype.is_floating_point else _PAT_ONE)
        body = b.raw[self.G: self.G + b.nbytes]
        prev = self._last.get((role, b.nbytes))
        if fill == FILL_LEFTOVERS and prev is not None and prev.raw.device == b.raw.device:
            body.copy_(prev.raw[self.G: self.G + b.nbytes])
            self.leftover_hits += 1
        else:
            body.fill_(FILL_ONES if fill == FILL_LEFTOVERS else int(fill))
        self._last[(role, b.nbytes)] = b
        return b.view

    def buf(self, shape, dtype, device, role, fill=None):
        """Drop-in for ``ops._buf``: ``fill=None`` (the binding leaves the buffer uninitialised) gets this guard's body
        fill, a number is the caller's own initialisation and is kept."""
        self.sizes[role] = _nbytes(shape, dtype)[1]
        if self.short.get(role):
            # the memory stays whole (so nothing can run out of bounds), only the size the caller passes on shrinks
            assert fill is None and dtype == torch.uint8
            return self.alloc(shape, dtype, device, role=role)[: self.sizes[role] - self.short[role]]
        if fill is None:
            return self.alloc(shape, dtype, device, role=role)
        t = self.alloc(shape, dtype, device, fill=FILL_ZERO, role=role)
        if fill != 0:
            t.fill_(fill)
        return t

    def wrap(self, tensor, role="input"):
        """A copy of an input inside a guarded block (NaN guards for floats, zero guards for integers); the bytes are
        remembered so that ``check()`` also proves that nothing wrote into the input."""
        tensor = tensor.contiguous()
        b = self._block(tuple(tensor.shape), tensor.dtype, tensor.device, role,
                        _PAT_NAN if tensor.dtype.is_floating_point else _PAT_ZERO)
        b.view.copy_(tensor)
        b.copy = b.raw[self.G: self.G + b.nbytes].clone()
        return b.view

    def wrap_all(self, *tensors, role="input"):
        return [self.wrap(t, "%s %d" % (role, i)) for i, t in enumerate(tensors)]

    # -- checks ---------------------------------------------------------------------------------------------------
    def check(self, what=""):
        """Every guard byte of every block still holds its pattern and every wrapped input its bytes; raises GuardError
        naming the block, the side and the offset of the first damaged byte (front: relative to the first byte of the
        view, negative; back: relative to the first byte after it)."""
        if not self.blocks:
            return
        if self.blocks[0].raw.is_cuda:
            torch.cuda.synchronize()            # whatever stream the call under test ran on
        G, firsts = self.G, []
        for b in self.blocks:
            exp = self._expect(b.raw.device, b.pattern)[:G]
            bad = torch.cat([b.raw[:G] != exp, b.raw[G + b.nbytes:] != exp])
            if b.copy is not None:
                bad = torch.cat([bad, b.raw[G: G + b.nbytes] != b.copy])
            firsts.append(torch.where(bad.any(), bad.to(torch.uint8).argmax(), -1))
        firsts = torch.stack(firsts).cpu().tolist()                 # the one wait
        errors = []
        for b, i in zip(self.blocks, firsts):
            if i < 0:
                continue
            if i < G:
                errors.append("%s, front guard, first bad byte %d" % (b.role, i - G))
            elif i < 2 * G:
                errors.append("%s, back guard, first bad byte +%d" % (b.role, i - G))
            else:
                errors.append("%s, input changed by the call, first changed byte %d" % (b.role, i - 2 * G))
        if errors:
            raise GuardError((what + ": " if what else "") + "; ".join(errors))

    def release(self):
        """Forget every block (the tensors handed out stay valid as long as the caller holds them)."""
        self.blocks, self._last = [], {}


def install(monkeypatch, guard):
    """Routes every allocation of the binding through ``guard`` for the rest of the test."""
    from gnnrag_amd import ops
    monkeypatch.setattr(ops, "_buf", guard.buf)
    return guard
