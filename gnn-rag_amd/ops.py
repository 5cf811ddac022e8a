"""Tensor-level wrappers over the C ABI: device memory and streams come from
PyTorch-ROCm (plumbing), every computation is a call into libgnnrag_hip.so."""
from __future__ import annotations

import collections
import ctypes as C
import os
from typing import Optional

import numpy as np
import torch

from . import _lib


MATH_FP32, MATH_BF16X3, MATH_MIXED = 0, 1, 2
MATH_NAMES = {MATH_FP32: "fp32 (v_mfma_f32_16x16x4_f32, bit-exact fmaf chains)",
              MATH_BF16X3: "bf16x3 (exact 3-way bf16 split, 6 plane products on v_mfma_f32_16x16x32_bf16, fp32 accumulate)",
              MATH_MIXED: "mixed (per kernel the faster fp32-class form: bf16x3 - exact 3-way bf16 split, 6 plane products, "
                          "fp32 accumulate - for the relation tables and the self-block update, exact fp32 MFMA for the "
                          "small products)"}
# Math mode the wrappers below pass to the library (the library itself keeps no mode: it is an argument of
# every dense entry point).  GNNRAG_MATH=fp32|bf16x3|mixed sets the binding's default.
_default_math = {"fp32": MATH_FP32, "bf16x3": MATH_BF16X3, "mixed": MATH_MIXED}[os.environ.get("GNNRAG_MATH", "mixed")]


def set_dense_math(mode: int) -> int:
    """Default math mode of this binding's dense calls: MATH_FP32 (exact fp32 MFMA), MATH_BF16X3 (exact 3-way bf16
    split, six plane products, fp32 accumulate) or MATH_MIXED (per kernel the faster of the two; the default).
    Returns the old mode."""
    global _default_math
    if mode not in (MATH_FP32, MATH_BF16X3, MATH_MIXED):
        raise ValueError("unknown math mode %r" % (mode,))
    old, _default_math = _default_math, int(mode)
    return old


def get_dense_math() -> int:
    return _default_math


def _math(math: Optional[int]) -> int:
    return _default_math if math is None else int(math)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _chk(t: torch.Tensor, name: str, dtype=torch.float32, shape=None) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.GnnragError("%s must live on the GPU (got %s); there is no CPU path" % (name, t.device))
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        t = t.contiguous()
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    return t


def _buf(shape, dtype, device, role: str, fill=None) -> torch.Tensor:
    """Every device buffer this binding allocates for the library (outputs, workspaces, structure memory, scratch)
    comes from here: ``fill=None`` leaves it uninitialised, a number fills it.  ``role`` names the buffer (entry point:
    argument); nothing here reads it - the guarded allocator of the tests (tests/guarded.py) replaces this function and
    reports a damaged guard under that name."""
    if fill is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if fill == 0:
        return torch.zeros(shape, dtype=dtype, device=device)
    return torch.full(shape, fill, dtype=dtype, device=device)


_stage_buf = {"t": None}


def _pinned_stage(n: int) -> torch.Tensor:
    """Pinned int32 staging block of at least n elements (grown geometrically, reused across batches)."""
    t = _stage_buf["t"]
    if t is None or t.numel() < n:
        t = torch.empty(max(n, 1 << 20, 0 if t is None else 2 * t.numel()), dtype=torch.int32, pin_memory=True)
        _stage_buf["t"] = t
    return t


def _on_plan_device(plan: "CsrPlan", t: torch.Tensor, name: str) -> None:
    """The structure's raw device pointers are only valid on the GPU it was built on."""
    if t.device != plan.device and not (t.is_cuda and plan.device.index is None):
        raise _lib.GnnragError("%s lives on %s but the structure was built on %s" % (name, t.device, plan.device))


class CsrPlan:
    """Device-side destination-sorted structure of one batch (both directions).

    Built from the first three arrays of the reference batch tuple
    (``kb_adj_mat`` = heads, rels, tails, ..., ``gnn/dataset_load.py:527``).
    Replaces ``BaseGNNLayer.build_matrix`` (``base_gnn.py:19-51``)."""

    def __init__(self, heads, rels, tails, B: int, N: int, R1: int, device, validate: bool = True,
                 hrt_device: Optional[torch.Tensor] = None, rel_counts=None):
        """``rel_counts = (rel_total, rel_max)``: the sum and the maximum over the questions of the distinct relation ids
        among a question's facts, when the caller knows them (a fact cache does: data/fact_mat.BatchFacts.rel_counts) -
        the build then does NOT wait for its stream (``gnnrag_csr_build_counts``); ``status()`` runs the deferred
        device-side validation whenever wanted."""
        lib = _lib.load()
        if hrt_device is not None:
            # the batch builder's [3, F] int32 block is already on the GPU (data/fact_mat.DeviceFactCache)
            if (hrt_device.dtype != torch.int32 or hrt_device.dim() != 2 or hrt_device.shape[0] != 3
                    or not hrt_device.is_cuda or not hrt_device.is_contiguous()):
                raise ValueError("hrt_device must be a contiguous [3, F] int32 CUDA tensor")
            heads = rels = tails = None
            F = int(hrt_device.shape[1])
        else:
            heads = np.asarray(heads)
            rels = np.asarray(rels)
            tails = np.asarray(tails)
            F = int(heads.shape[0])
        if hrt_device is None and (rels.shape[0] != F or tails.shape[0] != F):
            raise ValueError("heads/rels/tails differ in length")
        if B <= 0 or N <= 0 or R1 <= 0:
            raise ValueError("B, N, R1 must be positive")
        if B * N >= 2 ** 31 or F >= 2 ** 31:
            raise ValueError("batch too large for int32 indices")
        # ranges and the no-fact-across-questions rule are checked on the device during the build, on the
        # int32-narrowed ids (GNNRAG_E_TUPLE -> ValueError below); `validate` is kept for API compatibility
        self.B, self.N, self.R1, self.F = int(B), int(N), int(R1), F
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.GnnragError("CsrPlan needs a GPU device, got %s" % self.device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        base = None if hrt_device is not None else heads.base
        if hrt_device is not None:
            if hrt_device.device != self.device and not (self.device.index is None):
                raise _lib.GnnragError("hrt_device lives on %s, the plan on %s" % (hrt_device.device, self.device))
            hrt = hrt_device if F else _buf((3, 1), torch.int32, hrt_device.device, "csr_build: heads/rels/tails (no facts)", 0)
        elif (F and isinstance(base, np.ndarray) and heads.dtype == np.int32 and base is rels.base
                and base is tails.base and base.dtype == np.int32 and base.shape == (3, F) and base.flags.c_contiguous
                and heads.ctypes.data == base[0].ctypes.data and rels.ctypes.data == base[1].ctypes.data
                and tails.ctypes.data == base[2].ctypes.data and heads.shape == rels.shape == tails.shape == (F,)
                and heads.strides == rels.strides == tails.strides == (4,)):
            hrt = base                  # the batch builder's own [3,F] int32 block (data/fact_mat.py): no copy
        elif (F and heads.dtype == rels.dtype == tails.dtype == np.int64 and heads.flags.c_contiguous
              and rels.flags.c_contiguous and tails.flags.c_contiguous):
            # the reference's own tuple (int64 arrays): threaded narrowing into a pinned staging block, with the
            # check that every id fits int32 (ids that wrapped could pass the device-side range check)
            stage = _pinned_stage(3 * F)
            rc = lib.gnnrag_narrow_tuple(heads.ctypes.data, rels.ctypes.data, tails.ctypes.data, F, stage.data_ptr(),
                                         min(8, os.cpu_count() or 1))
            if rc == _lib.E_TUPLE:
                raise ValueError("edge tuple out of range: ids must lie in [0, 2^31)")
            _lib.check(rc, "gnnrag_narrow_tuple")
            hrt = stage[: 3 * F].view(3, F)
        else:
            for name, a in (("heads", heads), ("rels", rels), ("tails", tails)):
                if F and a.dtype.itemsize > 4 and (int(a.max()) >= 2 ** 31 or int(a.min()) < 0):
                    raise ValueError("edge tuple out of range: %s holds ids outside [0, 2^31)" % name)
            hrt = np.empty((3, max(F, 1)), dtype=np.int32)
            hrt[0, :F], hrt[1, :F], hrt[2, :F] = heads, rels, tails
        with torch.cuda.device(self.device):
            if hrt_device is not None:
                self._hrt = hrt                                                         # already resident
            elif isinstance(hrt, np.ndarray):
                self._hrt = torch.from_numpy(hrt).to(self.device, non_blocking=False)   # ONE int32 upload
            else:
                self._hrt = hrt.to(self.device, non_blocking=True)                      # from the pinned block
                torch.cuda.current_stream().synchronize()                               # the block is reused next batch
            nbytes = lib.gnnrag_csr_bytes(F, B, N, R1, 0, 0)
            sbytes = lib.gnnrag_csr_scratch_bytes(F, B, N, R1)
            self._mem = _buf(max(nbytes, 256), torch.uint8, self.device, "csr_build: csr_mem")
            scratch = _buf(max(sbytes, 256), torch.uint8, self.device, "csr_build: scratch")
            self.c = _lib.CsrStruct()
            row = self._hrt
            rt, rm = (-1, -1) if rel_counts is None else (int(rel_counts[0]), int(rel_counts[1]))
            rc = lib.gnnrag_csr_build_counts(
                row[0].data_ptr(), row[1].data_ptr(), row[2].data_ptr(), None, None,
                F, B, N, R1, rt, rm, self._mem.data_ptr(), self._mem.numel(),
                scratch.data_ptr(), scratch.numel(), C.byref(self.c), _stream())
            if rel_counts is not None:
                scratch.record_stream(torch.cuda.current_stream())      # the build has not run yet: keep its scratch
            if rc == _lib.E_TUPLE:
                raise ValueError("edge tuple out of range: node ids must lie in [0, B*N), relation ids in [0, R1), "
                                 "and a fact may not connect two different questions")
            _lib.check(rc, "gnnrag_csr_build")
            # the build waits for its stream once (it returns the relation counts), so scratch is free
        self._w = {}
        # compact relation rows: question b's tables are rows rel_off[b] : rel_off[b+1] of P[d]
        self.rel_total, self.rel_max = int(self.c.rel_total), int(self.c.rel_max)

    def status(self) -> None:
        """The deferred check of a structure built with ``rel_counts`` (waits for the stream once): raises ``ValueError``
        for an invalid tuple, ``GnnragError`` when the counts passed in differ from what the device counted."""
        rc = _lib.load().gnnrag_csr_status(C.byref(self.c), _stream())
        if rc == _lib.E_TUPLE:
            raise ValueError("edge tuple out of range: node ids must lie in [0, B*N), relation ids in [0, R1), "
                             "and a fact may not connect two different questions")
        _lib.check(rc, "gnnrag_csr_status (relation counts passed to the build differ from the device's)")

    @classmethod
    def concat(cls, parts, N: int, R1: int, device) -> "CsrPlan":
        """The structure of a batch as the concatenation of per-question structures already on the device
        (``gnnrag_csr_concat``; ``parts`` = one ``CsrPlan(..., B=1, N, R1)`` per question, in batch order): a copy with
        offsets - no upload, no sort, no wait for the stream; bit-identical to building the batch tuple from scratch."""
        lib = _lib.load()
        B = len(parts)
        if B == 0:
            raise ValueError("a batch needs at least one question")
        self = cls.__new__(cls)
        self.B, self.N, self.R1 = B, int(N), int(R1)
        self.F = int(sum(p.F for p in parts))
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        for p in parts:
            if p.B != 1 or p.N != self.N or p.R1 != self.R1 or p.device != self.device:
                raise ValueError("parts must be single-question structures of the same N / R1 on %s" % self.device)
        if B * self.N >= 2 ** 31 or self.F >= 2 ** 31:
            raise ValueError("batch too large for int32 indices")
        arr = (C.POINTER(_lib.CsrStruct) * B)(*[C.pointer(p.c) for p in parts])
        with torch.cuda.device(self.device):
            nbytes = lib.gnnrag_csr_bytes(self.F, B, self.N, self.R1, 0, 0)
            self._mem = _buf(max(nbytes, 256), torch.uint8, self.device, "csr_concat: csr_mem")
            self.c = _lib.CsrStruct()
            _lib.check(lib.gnnrag_csr_concat(arr, B, self.N, self.R1, self._mem.data_ptr(), self._mem.numel(),
                                             C.byref(self.c), _stream()), "gnnrag_csr_concat")
        self._parts = list(parts)            # the per-question blocks stay alive as long as the batch may read them
        self._hrt_lazy = None
        self._w = {}
        self.rel_total, self.rel_max = int(self.c.rel_total), int(self.c.rel_max)
        return self

    @property
    def _hrt(self):
        """[3, F] int32 id block of the batch tuple on the device (the backward's (question, relation) ordering reads
        it).  A concatenated structure builds it from its parts on first use."""
        if getattr(self, "_hrt_lazy", None) is None:
            blocks = []
            for b, p in enumerate(self._parts):
                h = p._hrt[:, : p.F].clone()
                h[0] += b * self.N
                h[2] += b * self.N
                blocks.append(h)
            self._hrt_lazy = (torch.cat(blocks, dim=1) if self.F else
                              _buf((3, 1), torch.int32, self.device, "relorder_build: heads/rels/tails (no facts)", 0))
        return self._hrt_lazy

    @_hrt.setter
    def _hrt(self, value):
        self._hrt_lazy = value

    def walk_workspace(self, D: int, I: int) -> torch.Tensor:
        """Scratch for the heavy-row partial sums of the walk kernels (cached per (D, I))."""
        key = ("ws", D, min(I, 3))
        if key not in self._w:
            nbytes = _lib.load().gnnrag_aggregate_workspace_bytes(C.byref(self.c), D, I)
            self._w[key] = _buf(max(nbytes, 256), torch.uint8, self.device, "aggregate / typelayer: workspace")
        return self._w[key]

    def relorder(self):
        """Facts ordered by (question, relation) for the backward's gather kernels; built on first use
        (training only).  Returns the ctypes struct (device arrays are owned by the plan)."""
        if ("relorder",) not in self._w:
            lib = _lib.load()
            w = self._w.get(("w_gnn_src",))
            with torch.cuda.device(self.device):
                mem = _buf(max(lib.gnnrag_relorder_bytes(C.byref(self.c), int(w is not None)), 256),
                           torch.uint8, self.device, "relorder_build: mem")
                scratch = _buf(max(lib.gnnrag_relorder_scratch_bytes(C.byref(self.c)), 256),
                               torch.uint8, self.device, "relorder_build: scratch")
                ro = _lib.RelorderStruct()
                row = self._hrt
                _lib.check(lib.gnnrag_relorder_build(
                    C.byref(self.c), row[0].data_ptr(), row[1].data_ptr(), row[2].data_ptr(), _ptr(w),
                    mem.data_ptr(), mem.numel(), scratch.data_ptr(), scratch.numel(), C.byref(ro), _stream()),
                    "gnnrag_relorder_build")
            self._w[("relorder",)] = (ro, mem)
        return self._w[("relorder",)][0]

    def backward_workspace(self, D: int, I: int, ro=None) -> torch.Tensor:
        """Scratch of the backward kernels, cached per (D, I)."""
        key = ("bws", D, I, ro is not None)
        if key not in self._w:
            nbytes = _lib.load().gnnrag_backward_workspace_bytes(C.byref(self.c), None if ro is None else C.byref(ro),
                                                                 D, I)
            self._w[key] = _buf(max(nbytes, 256), torch.uint8, self.device, "backward: workspace")
        return self._w[key]

    # -- lazily attached per-fact weights ----------------------------------------------------
    def _attach(self, key: str, w_per_fact, square: bool):
        if key in self._w:
            return
        lib = _lib.load()
        w = np.asarray(w_per_fact, dtype=np.float32)
        if w.shape[0] != self.F:
            raise ValueError("%s has %d entries for %d facts" % (key, w.shape[0], self.F))
        with torch.cuda.device(self.device):
            src = torch.from_numpy(w).to(self.device) if self.F else _buf(1, torch.float32, self.device, "csr_permute_weight: w_per_fact (no facts)", 0)
            out = _buf((2, max(self.F, 1)), torch.float32, self.device, "csr_permute_weight: out")
            _lib.check(lib.gnnrag_csr_permute_weight(C.byref(self.c), src.data_ptr(), int(square),
                                                     out[0].data_ptr(), out[1].data_ptr(), _stream()),
                       "gnnrag_csr_permute_weight")
        self._w[key] = out
        if key == "w_gnn":
            if ("relorder",) in self._w:
                raise RuntimeError("attach_w_gnn after the backward structure was built")
            self._w[("w_gnn_src",)] = src            # original fact order: the (question, relation) ordering permutes it too
        if key == "w_rel":
            self._w[("w_rel_src",)] = src            # read through relorder.perm by the TypeLayer backward
        arr = getattr(self.c, key)
        arr[0], arr[1] = out[0].data_ptr(), out[1].data_ptr()

    def attach_w_gnn(self, weight_list):
        """``weight_list`` = 1/outdeg(head); used squared when ``normalized_gnn`` (base_gnn.py:38-47)."""
        self._attach("w_gnn", weight_list, True)

    def attach_w_rel(self, weight_rel_list):
        """``weight_rel_list`` = 1/count(head, rel); TypeLayer ``norm_rel`` (layer_init.py:39-40)."""
        self._attach("w_rel", weight_rel_list, False)

    # -- debug / test views --------------------------------------------------------------------
    def rel_rows_device(self) -> torch.Tensor:
        """[rel_total, 2] int32 (question, relation id) of every compact relation row, a view of the structure's own
        device memory (the differentiable relation tables of training index T and the instructions with it)."""
        if self.rel_total == 0:
            return torch.zeros((0, 2), dtype=torch.int32, device=self.device)
        off = int(C.cast(self.c.rel_rows, C.c_void_p).value) - self._mem.data_ptr()
        return self._mem[off: off + 8 * self.rel_total].view(torch.int32).view(-1, 2)

    def _view(self, addr: int, n: int, dtype):
        if n == 0:
            return torch.zeros(0, dtype=dtype)
        base = self._mem.data_ptr()
        off = addr - base
        nbytes = n * torch.empty(0, dtype=dtype).element_size()
        return self._mem[off: off + nbytes].view(dtype).cpu()

    def to_host(self) -> dict:
        """Copies the structure back (tests only)."""
        BN = self.B * self.N
        out = {}
        for d in (0, 1):
            out["row_ptr%d" % d] = self._view(self.c.row_ptr[d], BN + 1, torch.int32).numpy()
            out["edge%d" % d] = self._view(self.c.edge[d], 2 * self.F, torch.int32).numpy().reshape(-1, 2)
            out["perm%d" % d] = self._view(self.c.perm[d], self.F, torch.int32).numpy()
        nh = self._view(self.c.n_heavy, 2, torch.int32).numpy()
        out["n_heavy"] = nh
        for d in (0, 1):
            out["heavy%d" % d] = self._view(self.c.heavy[d], int(min(nh[d], self.c.heavy_cap)), torch.int32).numpy()
            out["hub_q_off%d" % d] = self._view(self.c.hub_q_off[d], self.B + 1, torch.int32).numpy()
            out["hub_wbase%d" % d] = self._view(self.c.hub_wbase[d], self.B + 1, torch.int32).numpy()
        for key, t in self._w.items():
            if isinstance(key, str):
                out[key] = t.cpu().numpy()
        nc = self._view(self.c.n_chunks, 2, torch.int32).numpy()
        out["n_chunks"] = nc
        bc = self._view(self.c.big_cnt, self.B, torch.int32).numpy()
        bn = self._view(self.c.big_nodes, BN, torch.int32).numpy().reshape(self.B, self.N)
        out["big"] = [np.sort(bn[b, : bc[b]]) for b in range(self.B)]
        for d in (0, 1):
            out["edge_l%d" % d] = self._view(self.c.edge_l[d], 2 * self.F, torch.int32).numpy().reshape(-1, 2)
        out["rel_off"] = self._view(self.c.rel_off, self.B + 1, torch.int32).numpy()
        out["rel_rows"] = self._view(self.c.rel_rows, 2 * self.rel_total, torch.int32).numpy().reshape(-1, 2)
        out["edge_m"] = self._view(self.c.edge_m, 4 * self.F, torch.int32).numpy().reshape(-1, 2)
        out["m_from"] = self._view(self.c.m_from, 2 * self.F, torch.int32).numpy()
        out["m_dst"] = self._view(self.c.m_dst, 2 * self.F, torch.int32).numpy()
        return out

    def rel_rows(self) -> np.ndarray:
        """[rel_total, 2] (question, relation id) of every compact relation row (host copy)."""
        return self._view(self.c.rel_rows, 2 * self.rel_total, torch.int32).numpy().reshape(-1, 2)


def linear(A: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor] = None,
           add: Optional[torch.Tensor] = None, relu: bool = False, math: Optional[int] = None) -> torch.Tensor:
    """act(A W^T + bias (+ add on the first add.shape[0] rows)) on fp32 MFMA."""
    lib = _lib.load()
    A = _chk(A, "A")
    W = _chk(W, "W")
    M, K = A.shape
    Nout = W.shape[0]
    if W.shape[1] != K:
        raise ValueError("W is %s, A is %s" % (tuple(W.shape), tuple(A.shape)))
    bias = None if bias is None else _chk(bias, "bias", shape=(Nout,))
    add_rows = 0
    if add is not None:
        add = _chk(add, "add")
        if add.shape[1] != Nout:
            raise ValueError("add must have %d columns" % Nout)
        add_rows = add.shape[0]
    out = _buf((M, Nout), torch.float32, A.device, "linear: out")
    with torch.cuda.device(A.device):
        _lib.check(lib.gnnrag_linear(A.data_ptr(), M, K, W.data_ptr(), _ptr(bias), _ptr(add), add_rows,
                                     int(relu), out.data_ptr(), Nout, _math(math), _stream()), "gnnrag_linear")
    return out


SplitkPlan = collections.namedtuple("SplitkPlan", "splits k_chunk launches")


def linear_splitk_plan(M: int, K: int, Nout: int, splits: int = 0) -> SplitkPlan:
    """``gnnrag_linear_splitk_plan`` (host only, no device): the effective ``(splits, k_chunk)`` and the launches of a
    ``linear_splitk`` call.  ``splits=0`` is the library's rule - a function of ``(K, Nout)`` alone, never of ``M``; a
    value >= 1 is forced.  A shape or a forced value the library refuses raises ``GnnragError`` with its code."""
    plan = _lib.SplitkPlanStruct()
    _lib.check(_lib.load().gnnrag_linear_splitk_plan(int(M), int(K), int(Nout), int(splits), C.byref(plan)),
               "gnnrag_linear_splitk_plan")
    return SplitkPlan(int(plan.splits), int(plan.k_chunk), int(plan.launches))


def linear_splitk(A: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor] = None, *, epi: str = "bias",
                  add: Optional[torch.Tensor] = None, ln=None, splits: int = 0,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``gnnrag_linear_splitk``: ``epilogue(A W^T + bias)`` with K cut into ``splits`` chunks across the chip and one
    deterministic reduce (exact fp32 MFMA; made for few rows).  ``epi``: ``"bias"``, ``"gelu"`` (erf) or ``"add_ln"`` =
    ``LayerNorm(x + add) g + b`` with ``ln = (g, b, eps)``.  ``out`` may be given, and for ``"add_ln"`` it may be ``add``
    itself.  A row of the result depends on its row of ``A`` (and ``add``) only, never on ``M``."""
    lib = _lib.load()
    if epi not in _lib.SPLITK_EPI:
        raise ValueError("epi must be one of %s" % (sorted(_lib.SPLITK_EPI),))
    A = _chk(A, "A")
    W = _chk(W, "W")
    if A.dim() != 2 or W.dim() != 2 or W.shape[1] != A.shape[1]:
        raise ValueError("W is %s, A is %s" % (tuple(W.shape), tuple(A.shape)))
    M, K = A.shape
    Nout = W.shape[0]
    bias = None if bias is None else _chk(bias, "bias", shape=(Nout,))
    g = b = None
    eps = 0.0
    if epi == "add_ln":
        if add is None or ln is None:
            raise ValueError("epi='add_ln' needs add and ln=(g, b, eps)")
        if not add.is_contiguous():
            raise ValueError("add must be contiguous")
        add = _chk(add, "add", shape=(M, Nout))
        g, b, eps = _chk(ln[0], "ln[0]", shape=(Nout,)), _chk(ln[1], "ln[1]", shape=(Nout,)), float(ln[2])
    elif add is not None or ln is not None:
        raise ValueError("add and ln belong to epi='add_ln'")
    if out is None:
        out = _buf((M, Nout), torch.float32, A.device, "linear_splitk: out")
    else:
        if not out.is_contiguous():
            raise ValueError("out must be contiguous")
        out = _chk(out, "out", shape=(M, Nout))
    nws = int(lib.gnnrag_linear_splitk_workspace_bytes(M, K, Nout, int(splits)))
    ws = _buf((max(nws, 16),), torch.uint8, A.device, "linear_splitk: workspace")
    with torch.cuda.device(A.device):
        _lib.check(lib.gnnrag_linear_splitk(A.data_ptr(), M, K, W.data_ptr(), _ptr(bias), _lib.SPLITK_EPI[epi], _ptr(add),
                                            _ptr(g), _ptr(b), eps, out.data_ptr(), Nout, int(splits), ws.data_ptr(),
                                            nws, _stream()), "gnnrag_linear_splitk")
    return out


def rel_transform(relfeat: torch.Tensor, relfeat_inv: torch.Tensor, layers, planes: bool = False, packed: bool = False):
    """Relation projections of all layers in one launch (reasongnn.py:75-79, :102-105):
    ``out[j, d] = rel_linear{j}(rel_features_d) (+ pos_emb{j}_d on its rows)``, d = 0 forward / 1 inverse.
    ``layers``: sequence of (W_rel [D,D], b_rel [D], pos_emb.weight or None, pos_emb_inv.weight or None).
    Returns [L, 2, R1, D]; with ``planes=True`` also the bf16 planes of relu(+-T) ([L, 2, 3, R1, 448] int16 view) that
    :func:`relation_tables_planes` multiplies; with ``packed=True`` instead the packed sparse operand (planes of abs(T) and
    sign bits, [L, 2, R1, 1408] uint8, include/gnnrag.h) that :func:`relation_tables_packed` multiplies."""
    if planes and packed:
        raise ValueError("planes and packed are two forms of the same operand: ask for one")
    lib = _lib.load()
    relfeat = _chk(relfeat, "rel_features")
    R1, D = relfeat.shape
    relfeat_inv = _chk(relfeat_inv, "rel_features_inv", shape=(R1, D))
    L = len(layers)
    params = (_lib.LayerParams * max(L, 1))()
    keep, pos_rows = [], 0
    for j, (W, b, pos, pos_inv) in enumerate(layers):
        W = _chk(W, "rel_linear.weight", shape=(D, D))
        b = _chk(b, "rel_linear.bias", shape=(D,))
        keep += [W, b]
        params[j].W_rel, params[j].b_rel = W.data_ptr(), b.data_ptr()
        if pos is not None:
            pos = _chk(pos, "pos_emb.weight")
            pos_inv = _chk(pos_inv, "pos_emb_inv.weight", shape=tuple(pos.shape))
            if pos.shape[1] != D or (pos_rows and pos.shape[0] != pos_rows):
                raise ValueError("pos_emb must be [rows, D], the same size in every layer")
            pos_rows = pos.shape[0]
            keep += [pos, pos_inv]
            params[j].pos_fwd, params[j].pos_inv = pos.data_ptr(), pos_inv.data_ptr()
    out = _buf((L, 2, R1, D), torch.float32, relfeat.device, "rel_transform: out")
    pl = None
    if planes:
        nbytes = lib.gnnrag_rel_planes_bytes(R1, D, L)
        if nbytes == 0:
            raise _lib.GnnragError("relation planes need a hidden size <= 224")
        pl = _buf((L, 2, 3, R1, nbytes // (L * 6 * R1 * 2)), torch.int16, relfeat.device, "rel_transform: planes")
    if packed:
        nbytes = lib.gnnrag_rel_packed_bytes(R1, D, L)
        if nbytes == 0:
            raise _lib.GnnragError("the packed relation operand needs a hidden size <= 224")
        pl = _buf((L, 2, R1, nbytes // (L * 2 * R1)), torch.uint8, relfeat.device, "rel_transform: packed")
    with torch.cuda.device(relfeat.device):
        if packed:
            _lib.check(lib.gnnrag_rel_transform_packed(relfeat.data_ptr(), relfeat_inv.data_ptr(), R1, D, L, params,
                                                       pos_rows, out.data_ptr(), _ptr(pl), _stream()),
                       "gnnrag_rel_transform_packed")
        else:
            _lib.check(lib.gnnrag_rel_transform(relfeat.data_ptr(), relfeat_inv.data_ptr(), R1, D, L, params, pos_rows,
                                                out.data_ptr(), _ptr(pl), _stream()), "gnnrag_rel_transform")
    return (out, pl) if planes or packed else out


def relation_tables_planes(plan: "CsrPlan", planes: torch.Tensor, ins: torch.Tensor, W_e2e: torch.Tensor) -> torch.Tensor:
    """Relation tables of ONE layer in the bf16x3 math mode from its pre-split relation planes (``rel_transform(...,
    planes=True)[1][j]``, [2, 3, R1, 448] int16): ``gnnrag_relation_tables_planes``.  Raises outside the kernel's
    shapes (193 <= D <= 208, rel_total >= 1024)."""
    lib = _lib.load()
    ins = _chk(ins, "relational_ins")
    B, I, D = ins.shape
    if (planes.dtype != torch.int16 or tuple(planes.shape[:3]) != (2, 3, plan.R1) or not planes.is_contiguous()
            or B != plan.B):
        raise ValueError("planes must be a contiguous [2, 3, R1, 448] int16 tensor of this plan's relation count")
    W_e2e = _chk(W_e2e, "e2e_linear.weight", shape=(D, (2 * I + 1) * D))
    _on_plan_device(plan, ins, "relational_ins")
    P = _buf((2, max(plan.rel_total, 1), D), torch.float32, ins.device, "relation_tables_planes: P")
    with torch.cuda.device(ins.device):
        _lib.check(lib.gnnrag_relation_tables_planes(C.byref(plan.c), planes.data_ptr(), ins.data_ptr(), W_e2e.data_ptr(),
                                                     P.data_ptr(), D, I, _stream()), "gnnrag_relation_tables_planes")
    return P[:, :plan.rel_total]


def relation_tables_packed(plan: "CsrPlan", packed: torch.Tensor, ins: torch.Tensor, W_e2e: torch.Tensor,
                           only_dir: int = -1) -> torch.Tensor:
    """:func:`relation_tables_planes` on ONE layer's packed operand (``rel_transform(..., packed=True)[1][j]``,
    [2, R1, 1408] uint8): ``gnnrag_relation_tables_packed``, the form the layer sequence runs - the same P bit for bit.
    ``only_dir`` 0 / 1: that direction's tables alone; the other half of the result is zeros."""
    lib = _lib.load()
    ins = _chk(ins, "relational_ins")
    B, I, D = ins.shape
    if (packed.dtype != torch.uint8 or packed.dim() != 3 or tuple(packed.shape[:2]) != (2, plan.R1)
            or not packed.is_contiguous() or B != plan.B):
        raise ValueError("packed must be a contiguous [2, R1, 1408] uint8 tensor of this plan's relation count")
    if only_dir not in (-1, 0, 1):
        raise ValueError("only_dir is -1, 0 or 1")
    W_e2e = _chk(W_e2e, "e2e_linear.weight", shape=(D, (2 * I + 1) * D))
    _on_plan_device(plan, ins, "relational_ins")
    P = _buf((2, max(plan.rel_total, 1), D), torch.float32, ins.device, "relation_tables_packed: P")
    if only_dir >= 0:
        P.zero_()
    with torch.cuda.device(ins.device):
        _lib.check(lib.gnnrag_relation_tables_packed(C.byref(plan.c), packed.data_ptr(), ins.data_ptr(), W_e2e.data_ptr(),
                                                     P.data_ptr(), D, I, only_dir, _stream()), "gnnrag_relation_tables_packed")
    return P[:, :plan.rel_total]


def gemm_tn(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """``A^T @ B`` for two row-major operands with the same (large) row count - the weight gradient of a dense
    projection, ``dW = dY^T X`` (``gnnrag_gemm_tn``: exact fp32 MFMA, fixed summation order)."""
    lib = _lib.load()
    A = _chk(A, "A")
    B = _chk(B, "B")
    if A.dim() != 2 or B.dim() != 2 or A.shape[0] != B.shape[0]:
        raise ValueError("A is %s, B is %s" % (tuple(A.shape), tuple(B.shape)))
    M, N1 = A.shape
    N2 = B.shape[1]
    out = _buf((N1, N2), torch.float32, A.device, "gemm_tn: C")
    with torch.cuda.device(A.device):
        # the chunk count behind the workspace size depends on the CURRENT device's CU count: query it on A's device
        ws = _buf(max(lib.gnnrag_gemm_tn_workspace_bytes(M, N1, N2), 16), torch.uint8, A.device, "gemm_tn: workspace")
        _lib.check(lib.gnnrag_gemm_tn(A.data_ptr(), B.data_ptr(), M, N1, N2, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                      _stream()), "gnnrag_gemm_tn")
    return out


def aggregate(plan: CsrPlan, dist: torch.Tensor, ins: torch.Tensor, T_fwd: torch.Tensor,
              T_inv: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    B, N = plan.B, plan.N
    ins = _chk(ins, "ins")
    _, I, D = ins.shape
    dist = _chk(dist, "dist").reshape(-1)
    _on_plan_device(plan, dist, "dist")
    if dist.numel() != B * N or ins.shape[0] != B:
        raise ValueError("dist/ins do not match the plan (B=%d, N=%d)" % (B, N))
    T_fwd = _chk(T_fwd, "T_fwd", shape=(plan.R1, D))
    T_inv = _chk(T_inv, "T_inv", shape=(plan.R1, D))
    agg = _buf((B * N, 2 * I * D), torch.float32, dist.device, "aggregate: agg")
    ws = plan.walk_workspace(D, I)
    with torch.cuda.device(dist.device):
        _lib.check(lib.gnnrag_aggregate(C.byref(plan.c), dist.data_ptr(), ins.data_ptr(), T_fwd.data_ptr(),
                                        T_inv.data_ptr(), agg.data_ptr(), D, I, ws.data_ptr(), ws.numel(),
                                        _stream()), "gnnrag_aggregate")
    return agg


def relation_tables(plan: CsrPlan, T_fwd: torch.Tensor, T_inv: torch.Tensor, ins: torch.Tensor,
                    W_e2e: torch.Tensor, math: Optional[int] = None) -> torch.Tensor:
    """P[d,row(b,r),:] = sum_i W_e2e[:, block(i,d)] relu(T_d[r,:] * ins[b,i,:])  ->  [2,rel_total,D],
    one row per (question, relation the question uses) - ``plan.rel_rows()`` lists them."""
    lib = _lib.load()
    ins = _chk(ins, "ins")
    B, I, D = ins.shape
    if B != plan.B:
        raise ValueError("ins has %d questions, the plan %d" % (B, plan.B))
    T_fwd = _chk(T_fwd, "T_fwd", shape=(plan.R1, D))
    T_inv = _chk(T_inv, "T_inv", shape=(plan.R1, D))
    W_e2e = _chk(W_e2e, "e2e_linear.weight", shape=(D, (2 * I + 1) * D))
    P = _buf((2, plan.rel_total, D), torch.float32, ins.device, "relation_tables: P")
    with torch.cuda.device(ins.device):
        _lib.check(lib.gnnrag_relation_tables(C.byref(plan.c), T_fwd.data_ptr(), T_inv.data_ptr(), ins.data_ptr(),
                                              W_e2e.data_ptr(), P.data_ptr(), D, I, _math(math), _stream()),
                   "gnnrag_relation_tables")
    return P


def relation_tables_backward_supported(D: int, I: int) -> bool:
    """Whether ``gnnrag_relation_tables_backward`` takes the hidden size and instruction count (float4 loaders and one
    float4 column per thread of its reductions; torch's allocations satisfy the alignment rules)."""
    return 0 < D <= 1024 and D % 4 == 0 and 0 < I <= 8


def relation_tables_backward(plan: CsrPlan, T_fwd: torch.Tensor, T_inv: torch.Tensor, ins: torch.Tensor,
                             W_e2e: torch.Tensor, g_P: torch.Tensor, math: Optional[int] = None, need_T_fwd: bool = True,
                             need_T_inv: bool = True, need_ins: bool = True, need_W: bool = True) -> dict:
    """Backward of :func:`relation_tables` (``gnnrag_relation_tables_backward``) from g_P [2,rel_total,D]; the other
    operands as the forward was given them.  Returns a dict: ``g_T_fwd`` / ``g_T_inv`` [R1,D] (a relation no question
    uses: +0), ``g_ins`` [B,I,D] (a question without facts: +0), ``g_W`` [D,(2I+1)D] (the self block, columns < D: +0);
    None where not wanted (its launches are then not made; all four unwanted is refused by the library).  relu(T * ins)
    is never stored, the gate is the product > 0.  One fixed summation order: the same bits every time."""
    lib = _lib.load()
    ins = _chk(ins, "ins")
    if ins.dim() != 3 or ins.shape[0] != plan.B:
        raise ValueError("ins is %s, the plan has %d questions" % (tuple(ins.shape), plan.B))
    B, I, D = ins.shape
    _on_plan_device(plan, ins, "ins")
    K = (2 * I + 1) * D
    T_fwd = _chk(T_fwd, "T_fwd", shape=(plan.R1, D))
    T_inv = _chk(T_inv, "T_inv", shape=(plan.R1, D))
    W_e2e = _chk(W_e2e, "e2e_linear.weight", shape=(D, K))
    g_P = _chk(g_P, "g_P", shape=(2, plan.rel_total, D))
    dev, role = ins.device, "relation_tables_backward: "
    out = {"g_T_fwd": _buf((plan.R1, D), torch.float32, dev, role + "g_T_fwd") if need_T_fwd else None,
           "g_T_inv": _buf((plan.R1, D), torch.float32, dev, role + "g_T_inv") if need_T_inv else None,
           "g_ins": _buf((B, I, D), torch.float32, dev, role + "g_ins") if need_ins else None,
           "g_W": _buf((D, K), torch.float32, dev, role + "g_W") if need_W else None}
    if plan.rel_total == 0:                 # real pointers also where nothing is read (as for aggregate_fused)
        g_P = _buf((2, 1, D), torch.float32, dev, role + "g_P (empty batch)", fill=0)
    with torch.cuda.device(dev):
        # the size depends on the CURRENT device's CU count (gnnrag_gemm_tn's chunks inside): query it on ins' device
        ws = _buf(max(lib.gnnrag_relation_tables_backward_workspace_bytes(C.byref(plan.c), D, I), 16), torch.uint8, dev,
                  role + "workspace")
        _lib.check(lib.gnnrag_relation_tables_backward(C.byref(plan.c), T_fwd.data_ptr(), T_inv.data_ptr(), ins.data_ptr(),
                                                       W_e2e.data_ptr(), g_P.data_ptr(), _ptr(out["g_T_fwd"]),
                                                       _ptr(out["g_T_inv"]), _ptr(out["g_ins"]), _ptr(out["g_W"]), D, I,
                                                       _math(math), ws.data_ptr(), ws.numel(), _stream()),
                   "gnnrag_relation_tables_backward")
    return out


WALK_L2_GATHER, WALK_LDS_16, WALK_LDS_32 = 0, 1, 2
WALK_KERNEL_NAMES = {WALK_L2_GATHER: "k_walk_light_q / k_walk_light<FUSED> + hub kernels (table rows gathered from L2)",
                     WALK_LDS_16: "k_fact_prior_merged + k_walk_slice<FUSED,1> (16-column table slices in LDS, merged rows)",
                     WALK_LDS_32: "k_fact_prior_merged + k_walk_slice<FUSED,2> (32-column table slices in LDS, merged rows)"}


def aggregate_fused_variant(plan: CsrPlan, D: int) -> int:
    """Which kernel ``aggregate_fused`` runs for this structure and hidden size (WALK_*)."""
    v = _lib.load().gnnrag_aggregate_fused_variant(C.byref(plan.c), int(D))
    if v < 0:
        _lib.check(v, "gnnrag_aggregate_fused_variant")
    return v


DENSE_ENTRIES = {"linear": 0, "linear_pair": 1, "update_score": 2, "update_score_fused": 3,
                 # gnnrag_update_drop_train, and the masked input / weight gradient products of its backward
                 "update_drop": 4, "update_drop_dx": 5, "update_drop_dw": 6,
                 # gnnrag_relation_tables_backward, (rel_total, D, I) as (M, K, Nout): one of its 2 I equal products in
                 # front of the gate, and the weight gradient with the generated operand
                 "rel_tables_dx": 7, "rel_tables_dw": 8}
DENSE_MISALIGNED_A, DENSE_MISALIGNED_W, DENSE_MISALIGNED_C, DENSE_MISALIGNED_ADD, DENSE_MISALIGNED_A1 = 1, 2, 4, 8, 16
(DENSE_NONE, DENSE_SKINNY, DENSE_KTILED, DENSE_WRES, DENSE_UPDATE_SKINNY, DENSE_UPDATE_B3,
 DENSE_WIDE, DENSE_GEMM_TN) = range(8)
DENSE_EPI_LINEAR, DENSE_EPI_UPDATE, DENSE_EPI_KEEP = 0, 1, 2
DENSE_KERNEL_NAMES = {DENSE_NONE: "nothing launched", DENSE_SKINNY: "k_gemm_skinny", DENSE_KTILED: "k_gemm_f32",
                      DENSE_WRES: "k_gemm_wres", DENSE_UPDATE_SKINNY: "k_update_skinny", DENSE_UPDATE_B3: "k_update_b3",
                      DENSE_WIDE: "EPI_LINEAR column blocks + k_score_rows", DENSE_GEMM_TN: "k_gemm_tn (masked B)"}
DenseForm = collections.namedtuple("DenseForm", [n for n, _ in _lib.DenseFormStruct._fields_])


def dense_form(entry: str, M: int, K: int, Nout: int, math: Optional[int] = None, add_rows: Optional[int] = None,
               misaligned: int = 0, block: int = 0) -> DenseForm:
    """Which kernel a dense call runs (``gnnrag_dense_form``: host only, the launchers' own decision function).
    ``entry``: a key of DENSE_ENTRIES; the update entry points ("update_score", "update_score_fused", "update_drop" and
    the two products of its backward, "update_drop_dx" - blocks of g_h, then those of g_agg - and "update_drop_dw") pass
    (BN, D, I) as (M, K, Nout).  ``add_rows=None``: no ``add``.  ``misaligned``: OR of DENSE_MISALIGNED_* (operands
    that are not 16-byte aligned).  ``block``: column block of a call that makes several launches.
    Returns a :class:`DenseForm`: ``family`` (DENSE_*), and for k_gemm_f32 its template arguments ``nt, mt, v4, epi,
    math, nw`` with the runtime switches ``v4out, n0``; for k_gemm_wres ``nt, nc, has_add, kguard``."""
    out = _lib.DenseFormStruct()
    _lib.check(_lib.load().gnnrag_dense_form(DENSE_ENTRIES[entry], int(M), int(K), int(Nout), _math(math),
                                             int(add_rows is not None), int(add_rows or 0), int(misaligned), int(block),
                                             C.byref(out)), "gnnrag_dense_form")
    return DenseForm(*(getattr(out, n) for n in DenseForm._fields))


HUB_FORM_NONE, HUB_FORM_DENSE, HUB_FORM_CHUNKED = 0, 1, 2


def aggregate_fused_hub_form(plan: CsrPlan, D: int, I: int = 1) -> dict:
    """What the hub rows of a fused aggregation call do for this structure: the device-side decision of the gather walk
    (dense product or chunked fallback), read back.  ``I`` sizes the workspace as the layer call does
    (``gnnrag_aggregate_workspace_bytes(csr, D, I)``, softmax_layer.hip layer_ws)."""
    lib = _lib.load()
    ws = plan.walk_workspace(D, I)
    form = _buf(4, torch.int32, ws.device, "aggregate_fused_hub_form: form", 0)
    with torch.cuda.device(ws.device):
        _lib.check(lib.gnnrag_aggregate_fused_hub_form(C.byref(plan.c), int(D), ws.data_ptr(), ws.numel(), form.data_ptr(),
                                                       _stream()), "gnnrag_aggregate_fused_hub_form")
    f = form.cpu().tolist()
    return {"form": f[0], "hubs": (f[1], f[2]), "relation_ranges": f[3]}


def aggregate_fused(plan: CsrPlan, dist: torch.Tensor, P: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    B, N = plan.B, plan.N
    P = _chk(P, "P")
    D = P.shape[-1]
    if tuple(P.shape) != (2, plan.rel_total, D):
        raise ValueError("P must be [2, plan.rel_total, D]")
    dist = _chk(dist, "dist").reshape(-1)
    _on_plan_device(plan, dist, "dist")
    out = _buf((B * N, D), torch.float32, dist.device, "aggregate_fused: out")
    ws = plan.walk_workspace(D, 1)
    with torch.cuda.device(dist.device):
        _lib.check(lib.gnnrag_aggregate_fused(C.byref(plan.c), dist.data_ptr(), P.data_ptr(), out.data_ptr(), D,
                                              ws.data_ptr(), ws.numel(), _stream()), "gnnrag_aggregate_fused")
    return out


class Frontier:
    """The frontier of a sparse prior (``gnnrag_frontier_build``): the nodes reached by the facts that start at a node
    with ``dist != 0`` and the compact relation rows those facts use.  Test-side view of what
    ``GNNRAG_PATH_SEED_PRIOR`` does inside ``gnnrag_reason_layer`` / ``gnnrag_reason_stack``."""

    def __init__(self, plan: CsrPlan, dist: torch.Tensor):
        lib = _lib.load()
        self.plan = plan
        dist = _chk(dist, "dist").reshape(-1)
        _on_plan_device(plan, dist, "dist")
        if dist.numel() != plan.B * plan.N:
            raise ValueError("dist does not match the plan")
        self.dist = dist
        nbytes = max(lib.gnnrag_frontier_workspace_bytes(C.byref(plan.c)), 256)
        self.ws = _buf(nbytes, torch.uint8, dist.device, "frontier_build: fws")
        with torch.cuda.device(dist.device):
            _lib.check(lib.gnnrag_frontier_build(C.byref(plan.c), dist.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                                                 _stream()), "gnnrag_frontier_build")

    def read(self):
        """(number of listed nodes, number of listed relation rows, row gates uint8 [B*N]) - synchronises."""
        counts = (C.c_int32 * 2)()
        flags = np.zeros(self.plan.B * self.plan.N, dtype=np.uint8)
        with torch.cuda.device(self.dist.device):
            _lib.check(_lib.load().gnnrag_frontier_read(C.byref(self.plan.c), self.ws.data_ptr(), counts,
                                                        flags.ctypes.data, _stream()), "gnnrag_frontier_read")
        return int(counts[0]), int(counts[1]), flags

    def relation_tables(self, T_fwd, T_inv, ins, W_e2e, P: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The listed rows of P [2, rel_total, D] (the rest keeps what ``P`` held; NaN-filled when allocated here)."""
        ins = _chk(ins, "ins")
        B, I, D = ins.shape
        T_fwd = _chk(T_fwd, "T_fwd", shape=(self.plan.R1, D))
        T_inv = _chk(T_inv, "T_inv", shape=(self.plan.R1, D))
        W_e2e = _chk(W_e2e, "e2e_linear.weight", shape=(D, (2 * I + 1) * D))
        if P is None:
            P = _buf((2, max(self.plan.rel_total, 1), D), torch.float32, ins.device, "relation_tables_frontier: P", float("nan"))
        with torch.cuda.device(ins.device):
            _lib.check(_lib.load().gnnrag_relation_tables_frontier(
                C.byref(self.plan.c), self.ws.data_ptr(), T_fwd.data_ptr(), T_inv.data_ptr(), ins.data_ptr(),
                W_e2e.data_ptr(), P.data_ptr(), D, I, _stream()), "gnnrag_relation_tables_frontier")
        return P

    def aggregate(self, P: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """nbr rows of the listed nodes ([B*N, D]; unlisted rows keep what ``out`` held, zeros when allocated here)."""
        P = _chk(P, "P")
        D = P.shape[-1]
        if out is None:
            out = _buf((self.plan.B * self.plan.N, D), torch.float32, P.device, "aggregate_fused_frontier: out", 0)
        with torch.cuda.device(P.device):
            _lib.check(_lib.load().gnnrag_aggregate_fused_frontier(
                C.byref(self.plan.c), self.ws.data_ptr(), self.dist.data_ptr(), P.data_ptr(), out.data_ptr(), D,
                _stream()), "gnnrag_aggregate_fused_frontier")
        return out


FRONTIER_PARTS = ("counts", "row_flag", "rows", "tflag", "trows", "seeds", "seedinfo")


def frontier_layout(plan: CsrPlan) -> dict:
    """Byte offsets of the parts of a frontier workspace (``gnnrag_frontier_layout``), plus ``total``."""
    off = (C.c_uint64 * 8)()
    _lib.check(_lib.load().gnnrag_frontier_layout(C.byref(plan.c), off), "gnnrag_frontier_layout")
    return dict(zip(FRONTIER_PARTS + ("total",), (int(x) for x in off)))


def seed_prologue(plan: CsrPlan, dist: torch.Tensor, ws: torch.Tensor, relfeat: torch.Tensor, relfeat_inv: torch.Tensor,
                  layers, T_out: torch.Tensor, packed_out: Optional[torch.Tensor] = None,
                  zero_a: Optional[torch.Tensor] = None, zero_b: Optional[torch.Tensor] = None) -> bool:
    """What the layer stack launches in front of a seed layer (``gnnrag_seed_prologue``): the relation projections of
    ``layers`` (as :func:`rel_transform` takes them) into ``T_out [L, 2, R1, D]`` (+ ``packed_out [L, 2, R1, 1408]``
    uint8) and the frontier of ``dist`` into the frontier workspace ``ws`` (uint8), zeroing ``zero_a`` / ``zero_b`` on the
    way - one launch where that applies, else the two launches it stands for.  Test-side: every output is the caller's
    buffer.  Returns whether the one launch was taken."""
    lib = _lib.load()
    relfeat = _chk(relfeat, "rel_features")
    R1, D = relfeat.shape
    relfeat_inv = _chk(relfeat_inv, "rel_features_inv", shape=(R1, D))
    dist = _chk(dist, "dist").reshape(-1)
    _on_plan_device(plan, dist, "dist")
    if dist.numel() != plan.B * plan.N or R1 != plan.R1:
        raise ValueError("dist / rel_features do not match the plan")
    L = len(layers)
    params = (_lib.LayerParams * max(L, 1))()
    keep, pos_rows = [], 0
    for j, (W, b, pos, pos_inv) in enumerate(layers):
        W = _chk(W, "rel_linear.weight", shape=(D, D))
        b = _chk(b, "rel_linear.bias", shape=(D,))
        keep += [W, b]
        params[j].W_rel, params[j].b_rel = W.data_ptr(), b.data_ptr()
        if pos is not None:
            pos = _chk(pos, "pos_emb.weight")
            pos_inv = _chk(pos_inv, "pos_emb_inv.weight", shape=tuple(pos.shape))
            pos_rows = pos.shape[0]
            keep += [pos, pos_inv]
            params[j].pos_fwd, params[j].pos_inv = pos.data_ptr(), pos_inv.data_ptr()
    if T_out.dtype != torch.float32 or T_out.numel() < L * 2 * R1 * D or not T_out.is_contiguous():
        raise ValueError("T_out must be a contiguous float32 buffer of at least L*2*R1*D elements")
    if packed_out is not None and packed_out.numel() * packed_out.element_size() < lib.gnnrag_rel_packed_bytes(R1, D, L):
        raise ValueError("packed_out is smaller than gnnrag_rel_packed_bytes")
    if ws.numel() * ws.element_size() < lib.gnnrag_frontier_workspace_bytes(C.byref(plan.c)):
        raise ValueError("ws is smaller than gnnrag_frontier_workspace_bytes")
    for z in (zero_a, zero_b):
        if z is not None and (z.dtype != torch.float32 or not z.is_contiguous()):
            raise ValueError("zero_a / zero_b must be contiguous float32")
    combined = C.c_int32(0)
    with torch.cuda.device(dist.device):
        _lib.check(lib.gnnrag_seed_prologue(
            C.byref(plan.c), dist.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(), _ptr(zero_a),
            zero_a.numel() if zero_a is not None else 0, _ptr(zero_b), zero_b.numel() if zero_b is not None else 0,
            relfeat.data_ptr(), relfeat_inv.data_ptr(), D, L, params, pos_rows, T_out.data_ptr(), _ptr(packed_out),
            C.byref(combined), _stream()), "gnnrag_seed_prologue")
    return bool(combined.value)


def update_score_fused(h, nbr, W, b, w_s, b_s, mask, I: int, math: Optional[int] = None):
    lib = _lib.load()
    h = _chk(h, "h")
    BN, D = h.shape
    nbr = _chk(nbr, "nbr", shape=(BN, D))
    W = _chk(W, "W", shape=(D, (2 * I + 1) * D))
    b = _chk(b, "b", shape=(D,))
    w_s = _chk(w_s, "w_s").reshape(-1)
    b_s = _chk(b_s, "b_s").reshape(-1)
    mask = _chk(mask, "mask").reshape(-1)
    h_out = _buf(h.shape, torch.float32, h.device, "update_score_fused: h_out")
    score = _buf(BN, torch.float32, h.device, "update_score_fused: score")
    with torch.cuda.device(h.device):
        _lib.check(lib.gnnrag_update_score_fused(h.data_ptr(), nbr.data_ptr(), W.data_ptr(), b.data_ptr(),
                                                 w_s.data_ptr(), b_s.data_ptr(), mask.data_ptr(), h_out.data_ptr(),
                                                 score.data_ptr(), BN, D, I, _math(math), _stream()),
                   "gnnrag_update_score_fused")
    return h_out, score


def update_score(h, agg, W, b, w_s, b_s, mask, I: int, math: Optional[int] = None):
    lib = _lib.load()
    h = _chk(h, "h")
    BN, D = h.shape
    agg = _chk(agg, "agg", shape=(BN, 2 * I * D))
    W = _chk(W, "W", shape=(D, (2 * I + 1) * D))
    b = _chk(b, "b", shape=(D,))
    w_s = _chk(w_s, "w_s").reshape(-1)
    b_s = _chk(b_s, "b_s").reshape(-1)
    mask = _chk(mask, "mask").reshape(-1)
    if w_s.numel() != D or b_s.numel() != 1 or mask.numel() != BN:
        raise ValueError("score_func / mask shapes do not match")
    h_out = _buf(h.shape, torch.float32, h.device, "update_score: h_out")
    score = _buf(BN, torch.float32, h.device, "update_score: score")
    with torch.cuda.device(h.device):
        _lib.check(lib.gnnrag_update_score(h.data_ptr(), agg.data_ptr(), W.data_ptr(), b.data_ptr(),
                                           w_s.data_ptr(), b_s.data_ptr(), mask.data_ptr(), h_out.data_ptr(),
                                           score.data_ptr(), BN, D, I, _math(math), _stream()), "gnnrag_update_score")
    return h_out, score


def masked_softmax(score: torch.Tensor, B: int, N: int) -> torch.Tensor:
    lib = _lib.load()
    score = _chk(score, "score")
    if score.numel() != B * N:
        raise ValueError("score has %d entries, expected %d" % (score.numel(), B * N))
    dist = _buf((B, N), torch.float32, score.device, "masked_softmax: dist")
    with torch.cuda.device(score.device):
        _lib.check(lib.gnnrag_masked_softmax(score.data_ptr(), dist.data_ptr(), B, N, _stream()),
                   "gnnrag_masked_softmax")
    return dist


def typelayer(plan: CsrPlan, T: torch.Tensor, use_w_rel: bool) -> torch.Tensor:
    lib = _lib.load()
    T = _chk(T, "T")
    _on_plan_device(plan, T, "T")
    D = T.shape[1]
    if T.shape[0] != plan.R1:
        raise ValueError("T has %d rows, plan has R1=%d" % (T.shape[0], plan.R1))
    h0 = _buf((plan.B * plan.N, D), torch.float32, T.device, "typelayer: h0")
    ws = plan.walk_workspace(D, 1)
    with torch.cuda.device(T.device):
        _lib.check(lib.gnnrag_typelayer(C.byref(plan.c), T.data_ptr(), int(use_w_rel), h0.data_ptr(), D,
                                        ws.data_ptr(), ws.numel(), _stream()), "gnnrag_typelayer")
    return h0


def aggregate_backward(plan: CsrPlan, dist, ins, T_fwd, T_inv, g_agg, gather: bool = True):
    """Gradients of ``aggregate`` with respect to (dist, ins, T_fwd, T_inv).  ``gather``: table / instruction
    gradients by the atomic-free gather over (question, relation) rows (needs D % 4 == 0, I <= 4; builds the
    ordering on first use) instead of relation-bucketed LDS sums."""
    lib = _lib.load()
    B, N = plan.B, plan.N
    ins = _chk(ins, "ins")
    _, I, D = ins.shape
    dist = _chk(dist, "dist").reshape(-1)
    T_fwd = _chk(T_fwd, "T_fwd", shape=(plan.R1, D))
    T_inv = _chk(T_inv, "T_inv", shape=(plan.R1, D))
    g_agg = _chk(g_agg, "g_agg", shape=(B * N, 2 * I * D))
    g_dist = _buf(B * N, torch.float32, dist.device, "aggregate_backward: g_dist")
    g_ins = _buf(ins.shape, torch.float32, ins.device, "aggregate_backward: g_ins")
    g_Tf = _buf(T_fwd.shape, torch.float32, T_fwd.device, "aggregate_backward: g_T_fwd")
    g_Ti = _buf(T_inv.shape, torch.float32, T_inv.device, "aggregate_backward: g_T_inv")
    ro = plan.relorder() if (gather and D % 4 == 0 and I <= 4) else None
    ws = plan.backward_workspace(D, I, ro)
    with torch.cuda.device(dist.device):
        _lib.check(lib.gnnrag_aggregate_backward(
            C.byref(plan.c), None if ro is None else C.byref(ro), dist.data_ptr(), ins.data_ptr(), T_fwd.data_ptr(),
            T_inv.data_ptr(), g_agg.data_ptr(),
            g_dist.data_ptr(), g_ins.data_ptr(), g_Tf.data_ptr(), g_Ti.data_ptr(), D, I, ws.data_ptr(), ws.numel(),
            _stream()), "gnnrag_aggregate_backward")
    return g_dist, g_ins, g_Tf, g_Ti


def aggregate_fused_backward(plan: CsrPlan, dist, P, g_nbr):
    """Gradients of ``aggregate_fused`` with respect to (dist, P): g_dist [BN], g_P [2, rel_total, D]."""
    lib = _lib.load()
    P = _chk(P, "P")
    D = P.shape[-1]
    if tuple(P.shape) != (2, plan.rel_total, D) or D % 4:
        raise ValueError("P must be [2, plan.rel_total, D] with D % 4 == 0")
    dist = _chk(dist, "dist").reshape(-1)
    g_nbr = _chk(g_nbr, "g_nbr", shape=(plan.B * plan.N, D))
    g_dist = _buf(plan.B * plan.N, torch.float32, dist.device, "aggregate_fused_backward: g_dist")
    g_P = _buf(P.shape, torch.float32, P.device, "aggregate_fused_backward: g_P", 0 if plan.rel_total == 0 else None)
    ro = plan.relorder()
    ws = plan.backward_workspace(D, 1, ro)
    with torch.cuda.device(dist.device):
        _lib.check(lib.gnnrag_aggregate_fused_backward(
            C.byref(plan.c), C.byref(ro), dist.data_ptr(), P.data_ptr(), g_nbr.data_ptr(), g_dist.data_ptr(),
            g_P.data_ptr(), D, ws.data_ptr(), ws.numel(), _stream()), "gnnrag_aggregate_fused_backward")
    return g_dist, g_P


def typelayer_backward(plan: CsrPlan, g_pre: torch.Tensor, use_w_rel: bool, gather: bool = True) -> torch.Tensor:
    """Gradient of ``typelayer`` with respect to T; g_pre = gradient of the pre-activation [BN, D].
    ``gather``: atomic-free gather over (question, relation) rows (D % 4 == 0) instead of LDS sums."""
    lib = _lib.load()
    g_pre = _chk(g_pre, "g_pre")
    D = g_pre.shape[1]
    if g_pre.shape[0] != plan.B * plan.N:
        raise ValueError("g_pre has %d rows, the plan %d nodes" % (g_pre.shape[0], plan.B * plan.N))
    g_T = _buf((plan.R1, D), torch.float32, g_pre.device, "typelayer_backward: g_T")
    ro = plan.relorder() if (gather and D % 4 == 0) else None
    w_src = plan._w.get(("w_rel_src",)) if use_w_rel else None
    if use_w_rel and w_src is None:
        raise ValueError("use_w_rel needs attach_w_rel first")
    ws = plan.backward_workspace(D, 1, ro)
    with torch.cuda.device(g_pre.device):
        _lib.check(lib.gnnrag_typelayer_backward(C.byref(plan.c), None if ro is None else C.byref(ro), g_pre.data_ptr(),
                                                 _ptr(w_src), int(use_w_rel), g_T.data_ptr(), D, ws.data_ptr(),
                                                 ws.numel(), _stream()), "gnnrag_typelayer_backward")
    return g_T


class LayerWorkspace:
    """Scratch of gnnrag_reason_layer (T_fwd, T_inv, agg), reused across layer calls."""

    def __init__(self):
        self.key = None
        self.buf = None

    def get(self, plan: "CsrPlan", D, I, device) -> torch.Tensor:
        nbytes = max(_lib.load().gnnrag_layer_workspace_bytes(C.byref(plan.c), D, I), 256)
        if self.key != str(device) or self.buf is None or self.buf.numel() < nbytes:
            self.buf = None                      # release the old buffer before taking the new one
            self.buf = _buf(nbytes, torch.uint8, device, "reason_layer: workspace")
            self.key = str(device)
        return self.buf


def reason_layer(plan: CsrPlan, h, dist, ins, relfeat, relfeat_inv, W_rel, b_rel, W_e2e, b_e2e, w_score,
                 b_score, mask, pos=None, pos_inv=None, ws: Optional[LayerWorkspace] = None,
                 path: int = _lib.PATH_AUTO, math: Optional[int] = None):
    """One ReasonGNNLayer.forward (reasongnn.py:134-174) = ONE call into the library.
    Returns (h_out [B,N,D], score [B,N], dist_out [B,N])."""
    lib = _lib.load()
    B, N, R1 = plan.B, plan.N, plan.R1
    ins = _chk(ins, "ins")
    _, I, D = ins.shape
    h = _chk(h, "h").reshape(B * N, D)
    _on_plan_device(plan, h, "local_entity_emb")
    dist = _chk(dist, "dist").reshape(-1)
    mask = _chk(mask, "mask").reshape(-1)
    relfeat = _chk(relfeat, "rel_features", shape=(R1, D))
    relfeat_inv = _chk(relfeat_inv, "rel_features_inv", shape=(R1, D))
    W_rel = _chk(W_rel, "rel_linear.weight", shape=(D, D))
    b_rel = _chk(b_rel, "rel_linear.bias", shape=(D,))
    W_e2e = _chk(W_e2e, "e2e_linear.weight", shape=(D, (2 * I + 1) * D))
    b_e2e = _chk(b_e2e, "e2e_linear.bias", shape=(D,))
    w_score = _chk(w_score, "score_func.weight").reshape(-1)
    b_score = _chk(b_score, "score_func.bias").reshape(-1)
    if dist.numel() != B * N or mask.numel() != B * N or ins.shape[0] != B or w_score.numel() != D:
        raise ValueError("layer inputs do not match the plan (B=%d, N=%d, D=%d)" % (B, N, D))
    pos_rows = 0
    if pos is not None:
        pos = _chk(pos, "pos_emb.weight")
        pos_inv = _chk(pos_inv, "pos_emb_inv.weight", shape=tuple(pos.shape))
        pos_rows = pos.shape[0]
        if pos.shape[1] != D or pos_rows > R1:
            raise ValueError("pos_emb must be [<=R1, D]")
    ws = ws or LayerWorkspace()
    wbuf = ws.get(plan, D, I, h.device)
    h_out = _buf((B, N, D), torch.float32, h.device, "reason_layer: h_out")
    score = _buf((B, N), torch.float32, h.device, "reason_layer: score")
    dist_out = _buf((B, N), torch.float32, h.device, "reason_layer: dist_out")
    with torch.cuda.device(h.device):
        _lib.check(lib.gnnrag_reason_layer(
            C.byref(plan.c), h.data_ptr(), dist.data_ptr(), ins.data_ptr(), relfeat.data_ptr(),
            relfeat_inv.data_ptr(), W_rel.data_ptr(), b_rel.data_ptr(), _ptr(pos), _ptr(pos_inv), pos_rows,
            W_e2e.data_ptr(), b_e2e.data_ptr(), w_score.data_ptr(), b_score.data_ptr(), mask.data_ptr(),
            h_out.data_ptr(), score.data_ptr(), dist_out.data_ptr(), wbuf.data_ptr(), wbuf.numel(), D, I,
            int(path), _math(math), _stream()), "gnnrag_reason_layer")
    return h_out, score, dist_out


class LayerStack:
    """The L ``ReasonGNNLayer.forward`` calls of one ReaRev iteration (rearev.py:208-210) as ONE library call
    (``gnnrag_reason_stack``), optionally captured as a hipGraph and replayed (``gnnrag_reason_stack_capture``).

    Everything that does not change between the iterations of a batch is validated and turned into raw pointers once,
    here: the structure, the relation features, the layers' parameters, the mask and the output buffers
    (``h [L,B,N,D]``, ``score`` / ``dist [L,B,N]``: every layer's outputs are kept, the reference returns each of
    them to its caller).  ``run(h0, dist0, ins)`` then costs one ctypes call."""

    def __init__(self, plan: CsrPlan, relfeat, relfeat_inv, layers, w_score, b_score, mask, I: int,
                 path: int = _lib.PATH_AUTO, math: Optional[int] = None):
        """layers: list of (W_rel, b_rel, W_e2e, b_e2e, pos, pos_inv) tensors per layer (pos / pos_inv may be None)."""
        lib = _lib.load()
        B, N, R1 = plan.B, plan.N, plan.R1
        relfeat = _chk(relfeat, "rel_features")
        D = relfeat.shape[1]
        _on_plan_device(plan, relfeat, "rel_features")
        self.plan, self.B, self.N, self.D, self.I, self.L = plan, B, N, D, int(I), len(layers)
        self.path, self.math = int(path), _math(math)
        keep = [relfeat, _chk(relfeat_inv, "rel_features_inv", shape=(R1, D)),
                _chk(w_score, "score_func.weight").reshape(-1), _chk(b_score, "score_func.bias").reshape(-1),
                _chk(mask, "mask").reshape(-1)]
        if tuple(relfeat.shape) != (R1, D) or keep[2].numel() != D or keep[4].numel() != B * N:
            raise ValueError("layer stack inputs do not match the plan (B=%d, N=%d, R1=%d, D=%d)" % (B, N, R1, D))
        self._relfeat, self._relfeat_inv, self._ws, self._bs, self._mask = keep
        self._params = (_lib.LayerParams * self.L)()
        self.pos_rows = 0
        for j, (W_rel, b_rel, W_e2e, b_e2e, pos, pos_inv) in enumerate(layers):
            t = [_chk(W_rel, "rel_linear.weight", shape=(D, D)), _chk(b_rel, "rel_linear.bias", shape=(D,)),
                 _chk(W_e2e, "e2e_linear.weight", shape=(D, (2 * self.I + 1) * D)),
                 _chk(b_e2e, "e2e_linear.bias", shape=(D,))]
            if pos is not None:
                pos = _chk(pos, "pos_emb.weight")
                pos_inv = _chk(pos_inv, "pos_emb_inv.weight", shape=tuple(pos.shape))
                if pos.shape[1] != D or pos.shape[0] > R1 or (self.pos_rows and pos.shape[0] != self.pos_rows):
                    raise ValueError("pos_emb must be [<=R1, D], the same size in every layer")
                self.pos_rows = pos.shape[0]
                t += [pos, pos_inv]
            keep += t
            pr = self._params[j]
            pr.W_rel, pr.b_rel, pr.W_e2e, pr.b_e2e = (x.data_ptr() for x in t[:4])
            pr.pos_fwd, pr.pos_inv = (t[4].data_ptr(), t[5].data_ptr()) if pos is not None else (None, None)
        self._keep = keep                                        # the tensors behind the raw pointers stay alive
        self.device = relfeat.device
        # the stack-sized workspace: relation projections of all L layers up front in one launch
        nbytes = max(lib.gnnrag_stack_workspace_bytes(C.byref(plan.c), self.L, D, self.I), 256)
        self._ws_buf = _buf(nbytes, torch.uint8, self.device, "reason_stack: workspace")
        self._graph = self._graph_rest = None
        self.h = self.score = self.dist = None                   # graph mode: the fixed buffers of the captured sequence
        # the relation projections of the L layers depend on the parameters and the relation features only: the first
        # run of a forward computes them into the workspace, the runs of its later iterations reuse them
        # (GNNRAG_PATH_REUSE_PROJ).  A stack is bound to one batch (the module builds a new one per batch); a caller that
        # keeps one stack across forwards calls new_forward() at the start of each.
        self._proj_valid = False

    def new_forward(self):
        """The next run() recomputes the relation projections (start of a new forward / batch)."""
        self._proj_valid = False

    def _new_outputs(self):
        f32, dev, L, B, N, D = torch.float32, self.device, self.L, self.B, self.N, self.D
        return (_buf((L, B, N, D), f32, dev, "reason_stack: h_out"), _buf((L, B, N), f32, dev, "reason_stack: score"),
                _buf((L, B, N), f32, dev, "reason_stack: dist_out"))

    def _args(self, h0, dist0, ins, out, reuse=False):
        h, score, dist = out
        return (C.byref(self.plan.c), self.L, self._params, h0.data_ptr(), dist0.data_ptr(), ins.data_ptr(),
                self._relfeat.data_ptr(), self._relfeat_inv.data_ptr(), self.pos_rows, self._ws.data_ptr(),
                self._bs.data_ptr(), self._mask.data_ptr(), h.data_ptr(), score.data_ptr(),
                dist.data_ptr(), self._ws_buf.data_ptr(), self._ws_buf.numel(), self.D, self.I,
                self.path | (_lib.PATH_REUSE_PROJ if reuse else 0), self.math)

    def _inputs(self, h0, dist0, ins):
        h0 = _chk(h0, "local_entity_emb").reshape(self.B * self.N, self.D)
        dist0 = _chk(dist0, "dist").reshape(-1)
        ins = _chk(ins, "relational_ins", shape=(self.B, self.I, self.D))
        if dist0.numel() != self.B * self.N:
            raise ValueError("dist does not match the plan")
        _on_plan_device(self.plan, h0, "local_entity_emb")
        return h0, dist0, ins

    def run(self, h0, dist0, ins):
        """Runs the L layers; returns freshly allocated (h [L,B,N,D], score [L,B,N], dist [L,B,N])."""
        h0, dist0, ins = self._inputs(h0, dist0, ins)
        out = self._new_outputs()
        reuse = self._proj_valid and self.L > 1
        with torch.cuda.device(h0.device):
            _lib.check(_lib.load().gnnrag_reason_stack(*self._args(h0, dist0, ins, out, reuse), _stream()),
                       "gnnrag_reason_stack")
        self._proj_valid = True
        return out

    def capture(self, h0, dist0, ins):
        """Captures the sequence as a hipGraph over FIXED buffers (``self.h / score / dist``, allocated here): the
        node state is read from ``self.h[L-1]`` (the previous iteration's last layer; ``h0`` is copied there now),
        the prior from ``dist0`` and the instructions from ``ins`` - both are kept and read again by every replay, so
        rewrite them in place between replays (rearev.py:208,217-221).  An eager ``run`` must have happened before
        (launch attributes are raised on first use)."""
        if self.L < 2:
            raise ValueError("graph replay needs num_gnn >= 2 (layer 0 reads the buffer the last layer writes)")
        self.release_graph()
        self.h, self.score, self.dist = self._new_outputs()
        self.h[self.L - 1].copy_(h0.reshape(self.B, self.N, self.D))
        h0g, dist0, ins = self._inputs(self.h[self.L - 1], dist0, ins)
        g, g2 = C.c_void_p(), C.c_void_p()
        with torch.cuda.device(h0g.device):
            # stream capture is not allowed on the legacy default stream (torch's default): capture on a side stream
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                _lib.check(_lib.load().gnnrag_reason_stack_capture(
                    *self._args(h0g, dist0, ins, (self.h, self.score, self.dist)), _stream(), C.byref(g)),
                    "gnnrag_reason_stack_capture")
                # second graph: the same sequence WITHOUT the relation projections - the iterations 2..T of a forward
                # (the eager run every capture needs left them in the workspace; every replay of the first graph
                # rewrites them)
                _lib.check(_lib.load().gnnrag_reason_stack_capture(
                    *self._args(h0g, dist0, ins, (self.h, self.score, self.dist), reuse=True), _stream(), C.byref(g2)),
                    "gnnrag_reason_stack_capture")
            torch.cuda.current_stream().wait_stream(side)
        self._graph, self._graph_rest, self._graph_in = g, g2, (dist0, ins)

    def capture_rest(self, h_prev, dist0, ins):
        """Module path (``ReasonGNNLayer._forward_stack``, iterations 2..T of a forward): captures ONLY the sequence without
        the relation projections (the eager run of iteration 1 left them in the workspace) over fixed buffers - the node
        state in ``self.h[L-1]`` (``h_prev`` is copied there), the prior ``dist0`` (the reference hands the same seed
        tensor to every iteration, rearev.py:208) and an instruction buffer of this stack, refreshed by ``replay_rest``."""
        if self.L < 2:
            raise ValueError("graph replay needs num_gnn >= 2 (layer 0 reads the buffer the last layer writes)")
        if not self._proj_valid:
            raise RuntimeError("capture_rest() needs the projections of an eager run() in the workspace")
        self.release_graph()
        self.h, self.score, self.dist = self._new_outputs()
        self._ins_buf = _buf((self.B, self.I, self.D), torch.float32, self.device, "reason_stack_capture: ins")
        self.h[self.L - 1].copy_(h_prev.reshape(self.B, self.N, self.D))
        self._ins_buf.copy_(ins)
        h0g, dist0, insb = self._inputs(self.h[self.L - 1], dist0, self._ins_buf)
        g2 = C.c_void_p()
        with torch.cuda.device(h0g.device):
            side = torch.cuda.Stream()                            # no capture on the legacy default stream
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                _lib.check(_lib.load().gnnrag_reason_stack_capture(
                    *self._args(h0g, dist0, insb, (self.h, self.score, self.dist), reuse=True), _stream(), C.byref(g2)),
                    "gnnrag_reason_stack_capture")
            torch.cuda.current_stream().wait_stream(side)
        self._graph_rest, self._graph_in = g2, (dist0, insb)

    def replay_rest(self, h_prev, dist0, ins):
        """One replay of the graph of ``capture_rest``: ``h_prev`` must be the previous replay's / capture's last-layer
        state (``self.h[L-1]``; anything else is copied in), ``dist0`` the captured prior tensor, ``ins`` is copied into the
        captured instruction buffer.  Returns the fixed buffers (overwritten by the next replay)."""
        if getattr(self, "_graph_rest", None) is None:
            raise RuntimeError("capture_rest() first")
        if dist0.data_ptr() != self._graph_in[0].data_ptr():
            raise RuntimeError("replay_rest: the prior is not the captured tensor")
        if h_prev.data_ptr() != self.h[self.L - 1].data_ptr():
            self.h[self.L - 1].copy_(h_prev.reshape(self.B, self.N, self.D))
        self._ins_buf.copy_(ins)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().gnnrag_graph_launch(self._graph_rest, _stream()), "gnnrag_graph_launch")
        return self.h, self.score, self.dist

    def replay(self, first: bool = True):
        """Replays the captured sequence.  ``first=False``: the graph without the relation-projection launch (the later
        iterations of a forward; the first one's replay left the projections in the workspace)."""
        if self._graph is None:
            raise RuntimeError("capture() first")
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().gnnrag_graph_launch(self._graph if first or self.L < 2 else self._graph_rest, _stream()),
                       "gnnrag_graph_launch")
        return self.h, self.score, self.dist

    def release_graph(self):
        for name in ("_graph", "_graph_rest"):
            if getattr(self, name, None) is not None:
                _lib.load().gnnrag_graph_destroy(getattr(self, name))
                setattr(self, name, None)

    def __del__(self):
        try:
            self.release_graph()
        except Exception:
            pass


def lstm_forward(x, w_ih, w_hh, b_ih=None, b_hh=None, h0=None, c0=None, workspaces=None):
    """One-layer batch_first LSTM, torch.nn.LSTM semantics (lstm_encoder.py:27-36): x [B,T,E], w_ih [4H,E], w_hh [4H,H],
    biases [4H] or None, h0 / c0 [B,H] or None (zeros).  Returns (out [B,T,H], h_n [B,H], c_n [B,H]).
    ``workspaces``: a dict OWNED BY THE CALLER (``HipLSTM`` keeps one per module) in which the transposed-weight scratch
    is kept between calls, keyed by (device, stream); None = a fresh scratch for this call."""
    lib = _lib.load()
    x = _chk(x, "x")
    if x.dim() != 3:
        raise ValueError("x must be [B,T,E]")
    B, T, E = x.shape
    w_ih = _chk(w_ih.detach(), "w_ih")
    H = w_ih.shape[0] // 4
    w_ih = _chk(w_ih, "w_ih", shape=(4 * H, E))
    w_hh = _chk(w_hh.detach(), "w_hh", shape=(4 * H, H))
    b_ih = None if b_ih is None else _chk(b_ih.detach(), "b_ih", shape=(4 * H,))
    b_hh = None if b_hh is None else _chk(b_hh.detach(), "b_hh", shape=(4 * H,))
    h0 = None if h0 is None else _chk(h0, "h0", shape=(B, H))
    c0 = None if c0 is None else _chk(c0, "c0", shape=(B, H))
    dev = x.device
    out = _buf((B, T, H), torch.float32, dev, "lstm_forward: out")
    h_n = _buf((B, H), torch.float32, dev, "lstm_forward: h_n")
    c_n = _buf((B, H), torch.float32, dev, "lstm_forward: c_n")
    need = lib.gnnrag_lstm_workspace_bytes(E, H)
    # one workspace per (device, stream): two calls on different streams of one device must not share the transposed-weight
    # scratch (calls on one stream are ordered)
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    ws = workspaces.get(key) if workspaces is not None else None
    if ws is None or ws.numel() < need:
        ws = _buf(need, torch.uint8, dev, "lstm_forward: workspace")
        if workspaces is not None:
            workspaces[key] = ws
    with torch.cuda.device(dev):
        _lib.check(lib.gnnrag_lstm_forward(x.data_ptr(), w_ih.data_ptr(), w_hh.data_ptr(), _ptr(b_ih), _ptr(b_hh), _ptr(h0),
                                           _ptr(c0), out.data_ptr(), h_n.data_ptr(), c_n.data_ptr(), B, T, E, H,
                                           ws.data_ptr(), ws.numel(), _stream()), "gnnrag_lstm_forward")
    return out, h_n, c_n


def _lstm_args(x, w_ih, w_hh, b_ih, b_hh, h0, c0):
    x = _chk(x, "x")
    if x.dim() != 3:
        raise ValueError("x must be [B,T,E]")
    B, T, E = x.shape
    w_ih = _chk(w_ih.detach(), "w_ih")
    H = w_ih.shape[0] // 4
    w_ih = _chk(w_ih, "w_ih", shape=(4 * H, E))
    w_hh = _chk(w_hh.detach(), "w_hh", shape=(4 * H, H))
    b_ih = None if b_ih is None else _chk(b_ih.detach(), "b_ih", shape=(4 * H,))
    b_hh = None if b_hh is None else _chk(b_hh.detach(), "b_hh", shape=(4 * H,))
    h0 = None if h0 is None else _chk(h0, "h0", shape=(B, H))
    c0 = None if c0 is None else _chk(c0, "c0", shape=(B, H))
    return x, w_ih, w_hh, b_ih, b_hh, h0, c0, (B, T, E, H)


def lstm_forward_train(x, w_ih, w_hh, b_ih=None, b_hh=None, h0=None, c0=None, workspaces=None):
    """:func:`lstm_forward` for training (``gnnrag_lstm_forward_train``): the same kernel and the same bits in out / h_n /
    c_n, plus the reserve (activated gates and cell states of every step, a uint8 tensor of
    ``gnnrag_lstm_reserve_bytes``) that :func:`lstm_backward` reads.  The reserve is allocated per call and returned: it
    belongs to this forward, not to ``workspaces`` (which, as in :func:`lstm_forward`, only keeps the transposed-weight
    scratch and is refilled by every call).  Returns (out, h_n, c_n, reserve)."""
    lib = _lib.load()
    x, w_ih, w_hh, b_ih, b_hh, h0, c0, (B, T, E, H) = _lstm_args(x, w_ih, w_hh, b_ih, b_hh, h0, c0)
    dev = x.device
    out = _buf((B, T, H), torch.float32, dev, "lstm_forward_train: out")
    h_n = _buf((B, H), torch.float32, dev, "lstm_forward_train: h_n")
    c_n = _buf((B, H), torch.float32, dev, "lstm_forward_train: c_n")
    reserve = _buf(lib.gnnrag_lstm_reserve_bytes(B, T, H), torch.uint8, dev, "lstm_forward_train: reserve")
    need = lib.gnnrag_lstm_workspace_bytes(E, H)
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    ws = workspaces.get(key) if workspaces is not None else None
    if ws is None or ws.numel() < need:
        ws = _buf(need, torch.uint8, dev, "lstm_forward_train: workspace")
        if workspaces is not None:
            workspaces[key] = ws
    with torch.cuda.device(dev):
        _lib.check(lib.gnnrag_lstm_forward_train(x.data_ptr(), w_ih.data_ptr(), w_hh.data_ptr(), _ptr(b_ih), _ptr(b_hh),
                                                 _ptr(h0), _ptr(c0), out.data_ptr(), h_n.data_ptr(), c_n.data_ptr(), B, T, E,
                                                 H, reserve.data_ptr(), reserve.numel(), ws.data_ptr(), ws.numel(),
                                                 _stream()), "gnnrag_lstm_forward_train")
    return out, h_n, c_n, reserve


def lstm_backward(x, w_ih, w_hh, h0, c0, out, reserve, g_out=None, g_hn=None, g_cn=None, need_dx=True, need_db=True,
                  need_dh0=False, need_dc0=False):
    """Backward of :func:`lstm_forward_train` (``gnnrag_lstm_backward``): x, the weights and h0 / c0 (None = zeros) as
    given to the forward, ``out`` and ``reserve`` as it returned them; g_out [B,T,H], g_hn / g_cn [B,H] the incoming
    gradients (None = zeros).  Returns (dx, dw_ih, dw_hh, db, dh0, dc0); an output that is not wanted is None and is
    not computed.  db is the gradient of b_ih and of b_hh alike.  One fixed summation order: the same bits every time."""
    lib = _lib.load()
    x, w_ih, w_hh, _, _, h0, c0, (B, T, E, H) = _lstm_args(x, w_ih, w_hh, None, None, h0, c0)
    out = _chk(out, "out", shape=(B, T, H))
    reserve = _chk(reserve, "reserve", dtype=torch.uint8)
    g_out = None if g_out is None else _chk(g_out, "g_out", shape=(B, T, H))
    g_hn = None if g_hn is None else _chk(g_hn, "g_hn", shape=(B, H))
    g_cn = None if g_cn is None else _chk(g_cn, "g_cn", shape=(B, H))
    dev = x.device
    dx = _buf((B, T, E), torch.float32, dev, "lstm_backward: dx") if need_dx else None
    dw_ih = _buf((4 * H, E), torch.float32, dev, "lstm_backward: dw_ih")
    dw_hh = _buf((4 * H, H), torch.float32, dev, "lstm_backward: dw_hh")
    db = _buf((4 * H,), torch.float32, dev, "lstm_backward: db") if need_db else None
    dh0 = _buf((B, H), torch.float32, dev, "lstm_backward: dh0") if need_dh0 else None
    dc0 = _buf((B, H), torch.float32, dev, "lstm_backward: dc0") if need_dc0 else None
    with torch.cuda.device(dev):
        # the size depends on the CURRENT device's CU count (gnnrag_gemm_tn inside): query it on x's device
        ws = _buf(max(lib.gnnrag_lstm_backward_workspace_bytes(B, T, E, H), 16), torch.uint8, dev,
                  "lstm_backward: workspace")
        _lib.check(lib.gnnrag_lstm_backward(x.data_ptr(), w_ih.data_ptr(), w_hh.data_ptr(), _ptr(h0), _ptr(c0),
                                            out.data_ptr(), reserve.data_ptr(), reserve.numel(), _ptr(g_out), _ptr(g_hn),
                                            _ptr(g_cn), _ptr(dx), dw_ih.data_ptr(), dw_hh.data_ptr(), _ptr(db), _ptr(dh0),
                                            _ptr(dc0), B, T, E, H, ws.data_ptr(), ws.numel(), _stream()),
                   "gnnrag_lstm_backward")
    return dx, dw_ih, dw_hh, db, dh0, dc0


def seed_retrieve(seed_info: torch.Tensor, ent_emb: torch.Tensor) -> torch.Tensor:
    """sum_n seed_info[b,n] * ent_emb[b,n,:]  ->  [B,D] (query_update.py:40), reading only flagged rows."""
    lib = _lib.load()
    seed_info = _chk(seed_info, "seed_info")
    B, N = seed_info.shape
    ent_emb = _chk(ent_emb, "ent_emb")
    if ent_emb.dim() != 3 or ent_emb.shape[0] != B or ent_emb.shape[1] != N:
        raise ValueError("ent_emb must be [B,N,D] matching seed_info [B,N]")
    D = ent_emb.shape[2]
    out = _buf((B, D), torch.float32, ent_emb.device, "seed_retrieve: out")
    with torch.cuda.device(ent_emb.device):
        _lib.check(lib.gnnrag_seed_retrieve(seed_info.data_ptr(), ent_emb.data_ptr(), out.data_ptr(), B, N, D,
                                            _stream()), "gnnrag_seed_retrieve")
    return out


def query_reform(q_node: torch.Tensor, seed_info: torch.Tensor, ent_emb: torch.Tensor, W_r: torch.Tensor,
                 W_g: torch.Tensor) -> torch.Tensor:
    """``QueryReform.forward`` in one launch (query_update.py:26-44 with Fusion :6-16):
    ``fusion(q_node, seed_retrieve(seed_info, ent_emb))`` -> [B, D].  ``ent_emb`` [B, N, D'] with D' >= D = q_node's
    width: a zero-padded node state is read in place."""
    lib = _lib.load()
    q_node = _chk(q_node, "q_node")
    seed_info = _chk(seed_info, "seed_info")
    ent_emb = _chk(ent_emb, "ent_emb")
    W_r = _chk(W_r, "W_r")
    W_g = _chk(W_g, "W_g")
    B, D = q_node.shape
    N = seed_info.shape[1]
    if (seed_info.shape[0] != B or ent_emb.dim() != 3 or ent_emb.shape[0] != B or ent_emb.shape[1] != N
            or ent_emb.shape[2] < D):
        raise ValueError("query_reform: q_node [B,D], seed_info [B,N], ent_emb [B,N,>=D]")
    if tuple(W_r.shape) != (D, 3 * D) or tuple(W_g.shape) != (D, 3 * D):
        raise ValueError("query_reform: fusion weights must be [D, 3D]")
    out = _buf((B, D), torch.float32, q_node.device, "query_reform: out")
    with torch.cuda.device(q_node.device):
        _lib.check(lib.gnnrag_query_reform(q_node.data_ptr(), seed_info.data_ptr(), ent_emb.data_ptr(), ent_emb.shape[2],
                                           W_r.data_ptr(), W_g.data_ptr(), out.data_ptr(), B, N, D, _stream()),
                   "gnnrag_query_reform")
    return out


MAX_REFORMS, QUERY_REFORM_MAX_D = 8, 4096       # GNNRAG_MAX_REFORMS, GNNRAG_QUERY_REFORM_MAX_D (include/gnnrag.h)


def query_reform_backward_supported(D: int, n: int) -> bool:
    """Whether ``gnnrag_query_reform_train`` / ``gnnrag_query_reform_backward`` take the shape.  The backward's LDS need
    (5 D floats) stays inside a CU's 160 KB at the forward's limit, so the limits are the forward's."""
    return 0 < D <= QUERY_REFORM_MAX_D and 0 < n <= MAX_REFORMS


def _ent_in_place(ent_emb: torch.Tensor, B: int, N: int):
    """(tensor, row stride): a node state whose last dimension is contiguous and whose rows are evenly spaced (a
    zero-padded state, or the view ``padded[:, :, :D]`` of one) is read where it lies; anything else is copied."""
    ld = ent_emb.stride(1)
    if ent_emb.stride(2) == 1 and ld >= ent_emb.shape[2] and ent_emb.stride(0) == N * ld:
        return ent_emb, ld
    ent_emb = ent_emb.contiguous()
    return ent_emb, ent_emb.shape[2]


def _qr_args(qs, seed_info, W_rs, W_gs):
    n = len(qs)
    if n == 0 or len(W_rs) != n or len(W_gs) != n:
        raise ValueError("query_reform: qs, W_rs and W_gs must be lists of the same length >= 1")
    qs = [_chk(q.detach(), "qs[%d]" % j) for j, q in enumerate(qs)]
    if qs[0].dim() != 2:
        raise ValueError("query_reform: every q must be [B,D]")
    B, D = qs[0].shape
    seed_info = _chk(seed_info.detach(), "seed_info")
    if seed_info.dim() != 2 or seed_info.shape[0] != B:
        raise ValueError("query_reform: seed_info must be [B,N]")
    for j in range(n):
        _chk(qs[j], "qs[%d]" % j, shape=(B, D))
    W_rs = [_chk(w.detach(), "W_rs[%d]" % j, shape=(D, 3 * D)) for j, w in enumerate(W_rs)]
    W_gs = [_chk(w.detach(), "W_gs[%d]" % j, shape=(D, 3 * D)) for j, w in enumerate(W_gs)]
    return qs, seed_info, W_rs, W_gs, (B, seed_info.shape[1], D, n)


def _ptr_array(tensors):
    return (C.c_void_p * max(len(tensors), 1))(*[_ptr(t) for t in tensors])


def query_reform_train(qs, seed_info, ent_emb, W_rs, W_gs):
    """The ``n = len(qs)`` reforms of one ReaRev iteration (rearev.py:217-221) in one launch
    (``gnnrag_query_reform_train``): ``qs`` / ``W_rs`` / ``W_gs`` LISTS of the reforms' instructions [B,D] and Fusion weights
    [D,3D]; one seed_info [B,N] and one ent_emb [B,N,D'] (D' >= D; last dimension contiguous and evenly spaced rows: read in
    place by its row stride) for all of them.  Returns (out [n,B,D], reserve): ``out[j]`` carries the bits of
    :func:`query_reform` on reform j; the reserve (a uint8 tensor of ``gnnrag_query_reform_reserve_bytes``: the retrieved
    rows, ``W_r f`` and the gates) is allocated per call and belongs to this forward - :func:`query_reform_backward` reads it.
    A shape outside the library's limits raises ``GnnragError`` (GNNRAG_E_UNSUPPORTED)."""
    lib = _lib.load()
    qs, seed_info, W_rs, W_gs, (B, N, D, n) = _qr_args(qs, seed_info, W_rs, W_gs)
    if not ent_emb.is_cuda:
        _chk(ent_emb, "ent_emb")
    if ent_emb.dtype != torch.float32:
        raise TypeError("ent_emb must be torch.float32, got %s" % ent_emb.dtype)
    if ent_emb.dim() != 3 or ent_emb.shape[0] != B or ent_emb.shape[1] != N or ent_emb.shape[2] < D:
        raise ValueError("query_reform_train: q [B,D], seed_info [B,N], ent_emb [B,N,>=D]")
    ent_emb, ld = _ent_in_place(ent_emb.detach(), B, N)
    dev = qs[0].device
    out = _buf((n, B, D), torch.float32, dev, "query_reform_train: out")
    reserve = _buf(lib.gnnrag_query_reform_reserve_bytes(B, D, n), torch.uint8, dev, "query_reform_train: reserve")
    with torch.cuda.device(dev):
        _lib.check(lib.gnnrag_query_reform_train(_ptr_array(qs), seed_info.data_ptr(), ent_emb.data_ptr(), ld,
                                                 _ptr_array(W_rs), _ptr_array(W_gs), out.data_ptr(), reserve.data_ptr(),
                                                 reserve.numel(), B, N, D, n, _stream()), "gnnrag_query_reform_train")
    return out, reserve


QR_GRADS = ("dq", "dW_r", "dW_g", "d_ent")


def query_reform_backward(qs, seed_info, W_rs, W_gs, reserve, g_outs, need=None):
    """Backward of :func:`query_reform_train` (``gnnrag_query_reform_backward``): qs, seed_info and the weights as given to
    the forward, the reserve it returned, ``g_outs``: a list of n gradients [B,D] of ``out[j]``; a ``None`` entry means that
    reform's output was not used - nothing is computed for it and it adds nothing to ``d_ent``.  ``need``: a dict over
    ``QR_GRADS`` of what is wanted (None: all; ``dq`` / ``dW_r`` / ``dW_g`` take one bool or a list with one per reform).
    Returns a dict over ``QR_GRADS``: dq / dW_r / dW_g lists per reform ([B,D], [D,3D]; None where not wanted or where the
    reform's ``g_outs`` entry is None), d_ent [B,N,D] (every element written; None when not wanted).  One fixed summation
    order: the same bits every time."""
    lib = _lib.load()
    qs, seed_info, W_rs, W_gs, (B, N, D, n) = _qr_args(qs, seed_info, W_rs, W_gs)
    reserve = _chk(reserve, "reserve", dtype=torch.uint8)
    if len(g_outs) != n:
        raise ValueError("query_reform_backward: g_outs must have one entry (or None) per reform")
    g_outs = [None if g is None else _chk(g, "g_outs[%d]" % j, shape=(B, D)) for j, g in enumerate(g_outs)]
    need = {k: True for k in QR_GRADS} if need is None else need

    def per_reform(k):
        v = need.get(k)
        v = [bool(x) for x in v] if isinstance(v, (list, tuple)) else [bool(v)] * n
        return [w and g is not None for w, g in zip(v, g_outs)]

    dev = qs[0].device
    role = "query_reform_backward: "
    out = {"dq": [_buf((B, D), torch.float32, dev, role + "dq") if w else None for w in per_reform("dq")],
           "dW_r": [_buf((D, 3 * D), torch.float32, dev, role + "dW_r") if w else None for w in per_reform("dW_r")],
           "dW_g": [_buf((D, 3 * D), torch.float32, dev, role + "dW_g") if w else None for w in per_reform("dW_g")],
           "d_ent": _buf((B, N, D), torch.float32, dev, role + "d_ent") if need.get("d_ent") else None}
    with torch.cuda.device(dev):
        ws = _buf(max(lib.gnnrag_query_reform_backward_workspace_bytes(B, N, D, n), 16), torch.uint8, dev,
                  role + "workspace")
        _lib.check(lib.gnnrag_query_reform_backward(
            _ptr_array(qs), seed_info.data_ptr(), _ptr_array(W_rs), _ptr_array(W_gs), reserve.data_ptr(), reserve.numel(),
            _ptr_array(g_outs), _ptr_array(out["dq"]), _ptr_array(out["dW_r"]), _ptr_array(out["dW_g"]),
            _ptr(out["d_ent"]), B, N, D, n, ws.data_ptr(), ws.numel(), _stream()), "gnnrag_query_reform_backward")
    return out


LAYER_TAIL_MAX_D = 4096                         # GNNRAG_LAYER_TAIL_MAX_D (include/gnnrag.h)


def layer_tail_supported(D: int) -> bool:
    """Whether ``gnnrag_layer_tail_train`` / ``gnnrag_layer_tail_backward`` take the hidden size."""
    return 0 < D <= LAYER_TAIL_MAX_D


def _lt_keep(keep, rows: int, D: int, scale: float):
    if keep is None:
        return None, 1.0
    return _chk(keep, "keep", dtype=torch.uint8, shape=(rows, D)), float(scale)


def layer_tail_train(pre_a, pre_b, keep, scale, w, b, mask):
    """The tail of the reasoning layer under autograd (reasongnn.py:163-169; ``gnnrag_layer_tail_train``): pre_a [B*N,D] and
    pre_b (the same shape, or None) are the layer's pre-activations, ``keep`` [B*N,D] uint8 0/1 with ``scale`` the dropout
    in front of ``score_func`` (None: no dropout, scale taken as 1), w [D] / b [1] the score function, mask [B,N].  Returns
    (h [B*N,D] = relu(pre_a + pre_b), score [B,N], dist [B,N]); dist carries the bits of :func:`masked_softmax` of score.  A
    hidden size outside the library's limit raises ``GnnragError`` (GNNRAG_E_UNSUPPORTED)."""
    lib = _lib.load()
    mask = _chk(mask, "mask")
    if mask.dim() != 2:
        raise ValueError("layer_tail_train: mask must be [B,N]")
    B, N = mask.shape
    pre_a = _chk(pre_a, "pre_a")
    if pre_a.dim() != 2 or pre_a.shape[0] != B * N:
        raise ValueError("layer_tail_train: pre_a must be [B*N,D] for a mask [B,N]")
    D = pre_a.shape[1]
    pre_b = None if pre_b is None else _chk(pre_b, "pre_b", shape=(B * N, D))
    keep, scale = _lt_keep(keep, B * N, D, scale)
    w = _chk(w.reshape(-1), "w", shape=(D,))
    b = _chk(b.reshape(-1), "b", shape=(1,))
    dev, role = pre_a.device, "layer_tail_train: "
    h = _buf((B * N, D), torch.float32, dev, role + "h")
    score = _buf((B, N), torch.float32, dev, role + "score")
    dist = _buf((B, N), torch.float32, dev, role + "dist")
    with torch.cuda.device(dev):
        _lib.check(lib.gnnrag_layer_tail_train(pre_a.data_ptr(), _ptr(pre_b), _ptr(keep), scale, w.data_ptr(), b.data_ptr(),
                                               mask.data_ptr(), B, N, D, h.data_ptr(), score.data_ptr(), dist.data_ptr(),
                                               _stream()), "gnnrag_layer_tail_train")
    return h, score, dist


def layer_tail_backward(h, dist, keep, scale, w, g_h, g_dist, need_dw: bool = True, need_db: bool = True):
    """Backward of :func:`layer_tail_train` (``gnnrag_layer_tail_backward``): h and dist as it returned them, keep / scale / w
    as it was given them, g_h [B*N,D] and g_dist [B,N] the upstream gradients (either may be None: that output was not
    used; both None is refused by the library).  Returns a dict: ``g_pre`` [B*N,D] (the gradient of pre_a and of pre_b
    alike, every element written), ``dw`` [D] and ``db`` [1] (exactly 0) or None where not wanted.  One fixed summation
    order: the same bits every time."""
    lib = _lib.load()
    dist = _chk(dist, "dist")
    if dist.dim() != 2:
        raise ValueError("layer_tail_backward: dist must be [B,N]")
    B, N = dist.shape
    h = _chk(h, "h")
    if h.dim() != 2 or h.shape[0] != B * N:
        raise ValueError("layer_tail_backward: h must be [B*N,D] for a dist [B,N]")
    D = h.shape[1]
    keep, scale = _lt_keep(keep, B * N, D, scale)
    w = _chk(w.reshape(-1), "w", shape=(D,))
    g_h = None if g_h is None else _chk(g_h, "g_h", shape=(B * N, D))
    g_dist = None if g_dist is None else _chk(g_dist, "g_dist", shape=(B, N))
    dev, role = h.device, "layer_tail_backward: "
    out = {"g_pre": _buf((B * N, D), torch.float32, dev, role + "g_pre"),
           "dw": _buf((D,), torch.float32, dev, role + "dw") if need_dw else None,
           "db": _buf((1,), torch.float32, dev, role + "db") if need_db else None}
    with torch.cuda.device(dev):
        ws = _buf(max(lib.gnnrag_layer_tail_backward_workspace_bytes(B, N, D), 16), torch.uint8, dev, role + "workspace")
        _lib.check(lib.gnnrag_layer_tail_backward(h.data_ptr(), dist.data_ptr(), _ptr(keep), scale, w.data_ptr(), _ptr(g_h),
                                                  _ptr(g_dist), B, N, D, out["g_pre"].data_ptr(), _ptr(out["dw"]),
                                                  _ptr(out["db"]), ws.data_ptr(), ws.numel(), _stream()),
                   "gnnrag_layer_tail_backward")
    return out


def update_drop_supported(D: int, I: int) -> bool:
    """Whether ``gnnrag_update_drop_train`` / ``gnnrag_update_drop_backward`` take the hidden size and instruction count
    (float4 loaders and 4-byte keep loads: D % 4 == 0; torch's allocations satisfy the alignment rules)."""
    return D > 0 and I > 0 and D % 4 == 0 and (2 * I + 1) * D < 2 ** 31


def _ud_args(h, agg, keep, scale, W, who: str):
    h = _chk(h, "h")
    if h.dim() != 2:
        raise ValueError(who + ": h must be [B*N,D]")
    BN, D = h.shape
    agg = _chk(agg, "agg")
    if agg.dim() != 2 or agg.shape[0] != BN or agg.shape[1] == 0 or agg.shape[1] % (2 * D):
        raise ValueError(who + ": agg must be [B*N,2*I*D] for an h [B*N,D]")
    I = agg.shape[1] // (2 * D)
    K = (2 * I + 1) * D
    W = _chk(W, "W", shape=(D, K))
    if keep is None:
        scale = 1.0
    else:
        keep, scale = _chk(keep, "keep", dtype=torch.uint8, shape=(BN, K)), float(scale)
    return h, agg, keep, scale, W, BN, D, I, K


def update_drop_train(h, agg, keep, scale, W, b, math: Optional[int] = None):
    """``pre = linear_drop(cat(h, agg)) W^T + b`` (reasongnn.py:161-163 in training; ``gnnrag_update_drop_train``): h [B*N,D],
    agg [B*N,2*I*D], ``keep`` [B*N,(2I+1)D] uint8 0/1 in the concatenation's column order with ``scale`` = 1/(1-p) (None: no
    dropout, scale taken as 1), W [D,(2I+1)D], b [D].  The dropped operand is formed inside the product's tile loader and
    never stored.  Returns pre [B*N,D]."""
    lib = _lib.load()
    h, agg, keep, scale, W, BN, D, I, K = _ud_args(h, agg, keep, scale, W, "update_drop_train")
    b = _chk(b, "b", shape=(D,))
    pre = _buf((BN, D), torch.float32, h.device, "update_drop_train: pre")
    with torch.cuda.device(h.device):
        _lib.check(lib.gnnrag_update_drop_train(h.data_ptr(), agg.data_ptr(), _ptr(keep), scale, W.data_ptr(), b.data_ptr(),
                                                BN, D, I, pre.data_ptr(), _math(math), _stream()),
                   "gnnrag_update_drop_train")
    return pre


def update_drop_backward(g_pre, h, agg, keep, scale, W, need_h: bool = True, need_agg: bool = True, need_dW: bool = True,
                         need_db: bool = True, math: Optional[int] = None):
    """Backward of :func:`update_drop_train` (``gnnrag_update_drop_backward``) from g_pre [B*N,D]; h / agg / keep / scale / W
    as the forward was given them.  Returns a dict: ``g_h`` [B*N,D] and ``g_agg`` [B*N,2*I*D] (every element written, a
    dropped one exactly +0), ``dW`` [D,(2I+1)D], ``db`` [D]; None where not wanted (its launches are then not made; all
    four unwanted is refused by the library).  One fixed summation order: the same bits every time."""
    lib = _lib.load()
    h, agg, keep, scale, W, BN, D, I, K = _ud_args(h, agg, keep, scale, W, "update_drop_backward")
    g_pre = _chk(g_pre, "g_pre", shape=(BN, D))
    dev, role = h.device, "update_drop_backward: "
    out = {"g_h": _buf((BN, D), torch.float32, dev, role + "g_h") if need_h else None,
           "g_agg": _buf((BN, K - D), torch.float32, dev, role + "g_agg") if need_agg else None,
           "dW": _buf((D, K), torch.float32, dev, role + "dW") if need_dW else None,
           "db": _buf((D,), torch.float32, dev, role + "db") if need_db else None}
    with torch.cuda.device(dev):
        # the size depends on the CURRENT device's CU count (gnnrag_gemm_tn's chunks inside): query it on h's device
        ws = _buf(max(lib.gnnrag_update_drop_backward_workspace_bytes(BN, D, I), 16), torch.uint8, dev, role + "workspace")
        _lib.check(lib.gnnrag_update_drop_backward(g_pre.data_ptr(), h.data_ptr(), agg.data_ptr(), _ptr(keep), scale,
                                                   W.data_ptr(), BN, D, I, _ptr(out["g_h"]), _ptr(out["g_agg"]),
                                                   _ptr(out["dW"]), _ptr(out["db"]), ws.data_ptr(), ws.numel(), _math(math),
                                                   _stream()), "gnnrag_update_drop_backward")
    return out


TRAIN_METRICS_MAX_N = 16384                     # GNNRAG_TRAIN_METRICS_MAX_N (include/gnnrag.h)


def train_metrics_supported(B: int, N: int) -> bool:
    """Whether ``gnnrag_train_metrics`` takes the shape (a question's sort keys live in LDS)."""
    return B > 0 and 0 < N <= TRAIN_METRICS_MAX_N


def _kl_args(pred, teacher, label_valid, who: str):
    pred = _chk(pred, "pred")
    if pred.dim() != 2:
        raise ValueError(who + ": pred must be [B,N]")
    B, N = pred.shape
    teacher = _chk(teacher, "teacher", shape=(B, N))
    label_valid = _chk(label_valid.reshape(-1), "label_valid", shape=(B,))
    return pred, teacher, label_valid, B, N


def kl_loss_train(pred, teacher, label_valid):
    """``calc_loss_label`` with ``loss_type='kl'`` (rearev.py:156-160 over base_model.py:193-215; ``gnnrag_kl_loss_train``):
    pred, teacher [B,N], label_valid [B] or [B,1].  Returns (loss [1], reserve [B]): the batch-mean KL loss and the answer
    counts ``len_b`` the backward reads.  One fixed summation order: the same bits every time."""
    lib = _lib.load()
    pred, teacher, label_valid, B, N = _kl_args(pred, teacher, label_valid, "kl_loss_train")
    dev, role = pred.device, "kl_loss_train: "
    loss = _buf((1,), torch.float32, dev, role + "loss")
    reserve = _buf((B,), torch.float32, dev, role + "reserve")
    with torch.cuda.device(dev):
        ws = _buf(max(lib.gnnrag_kl_loss_workspace_bytes(B), 16), torch.uint8, dev, role + "workspace")
        _lib.check(lib.gnnrag_kl_loss_train(pred.data_ptr(), teacher.data_ptr(), label_valid.data_ptr(), B, N,
                                            loss.data_ptr(), reserve.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
                   "gnnrag_kl_loss_train")
    return loss, reserve


def kl_loss_backward(g_loss, pred, teacher, label_valid, reserve):
    """Backward of :func:`kl_loss_train` (``gnnrag_kl_loss_backward``): g_loss a device tensor of one element (it is never
    read on the host), reserve as the forward returned it.  Returns d_pred [B,N], every element written; exactly 0 where
    teacher == 0 or label_valid == 0.  teacher receives no gradient."""
    lib = _lib.load()
    pred, teacher, label_valid, B, N = _kl_args(pred, teacher, label_valid, "kl_loss_backward")
    g_loss = _chk(g_loss.reshape(-1), "g_loss", shape=(1,))
    reserve = _chk(reserve, "reserve", shape=(B,))
    d_pred = _buf((B, N), torch.float32, pred.device, "kl_loss_backward: d_pred")
    with torch.cuda.device(pred.device):
        _lib.check(lib.gnnrag_kl_loss_backward(g_loss.data_ptr(), pred.data_ptr(), teacher.data_ptr(),
                                               label_valid.data_ptr(), reserve.data_ptr(), B, N, d_pred.data_ptr(),
                                               _stream()), "gnnrag_kl_loss_backward")
    return d_pred


def train_metrics(pred, answer, seed, local_entity, pad_id: int, eps: float):
    """``get_eval_metric`` of a training step (base_model.py:217-298) in one launch (``gnnrag_train_metrics``): pred, answer,
    seed [B,N] float, local_entity [B,N] int64, pad_id the pad entity, eps the model's top-p bound.  Returns
    (out_pred int32 [B], h1 float [B], f1 float [B], counts int32 [B,4] = (kept, n_ret, correct, n_ans)); nothing is read on
    the host.  N beyond the library's limit raises ``GnnragError`` (GNNRAG_E_UNSUPPORTED)."""
    lib = _lib.load()
    pred = _chk(pred, "pred")
    if pred.dim() != 2:
        raise ValueError("train_metrics: pred must be [B,N]")
    B, N = pred.shape
    answer = _chk(answer, "answer", shape=(B, N))
    seed = _chk(seed, "seed", shape=(B, N))
    local_entity = _chk(local_entity, "local_entity", dtype=torch.int64, shape=(B, N))
    dev, role = pred.device, "train_metrics: "
    out_pred = _buf((B,), torch.int32, dev, role + "pred")
    h1 = _buf((B,), torch.float32, dev, role + "h1")
    f1 = _buf((B,), torch.float32, dev, role + "f1")
    cnt = _buf((B, 4), torch.int32, dev, role + "counts")
    with torch.cuda.device(dev):
        _lib.check(lib.gnnrag_train_metrics(pred.data_ptr(), answer.data_ptr(), seed.data_ptr(), local_entity.data_ptr(),
                                            int(pad_id), float(eps), B, N, out_pred.data_ptr(), h1.data_ptr(), f1.data_ptr(),
                                            cnt.data_ptr(), _stream()), "gnnrag_train_metrics")
    return out_pred, h1, f1, cnt


OPTIM_CHUNK = _lib.OPTIM_CHUNK                  # GNNRAG_OPTIM_CHUNK (include/gnnrag.h)
OPTIM_SEG_BYTES = C.sizeof(_lib.OptimSeg)
# numpy mirror of gnnrag_optim_seg: a table is filled column by column on the host (gnnrag_amd/optim.py)
OPTIM_SEG_DTYPE = np.dtype([(n, np.uint64) for n in ("p", "g", "m", "v")] + [("n", np.int64), ("first_chunk", np.int64)] +
                           [(n, np.float32) for n in ("beta1", "beta2", "om_beta1", "om_beta2", "eps", "weight_decay",
                                                      "step_size", "bc2_sqrt")])
assert OPTIM_SEG_DTYPE.itemsize == OPTIM_SEG_BYTES == 80


def optim_chunks(numels):
    """(first_chunk of every tensor, n_chunks) for tensors of ``numels`` elements: the prefix sums of
    ceil(n / GNNRAG_OPTIM_CHUNK) a segment table carries."""
    first, total = [], 0
    for n in numels:
        first.append(total)
        total += (int(n) + OPTIM_CHUNK - 1) // OPTIM_CHUNK
    return first, total


def _optim_table(segs, T: int, who: str) -> torch.Tensor:
    if not segs.is_cuda:
        raise _lib.GnnragError("%s: segs must live on the GPU (got %s); there is no CPU path" % (who, segs.device))
    if segs.dtype != torch.uint8 or not segs.is_contiguous() or segs.numel() < T * OPTIM_SEG_BYTES or T <= 0:
        raise ValueError("%s: segs must be a contiguous uint8 tensor of at least T * %d bytes, T > 0" % (who, OPTIM_SEG_BYTES))
    return segs


def grad_norm(segs: torch.Tensor, T: int, n_chunks: int, max_norm: float) -> torch.Tensor:
    """``clip_grad_norm_`` without the rescaling (``gnnrag_grad_norm``): segs a DEVICE table of T ``gnnrag_optim_seg`` entries
    as a uint8 tensor (``OPTIM_SEG_DTYPE``; only g, n and first_chunk are read), n_chunks from :func:`optim_chunks`.
    Returns out2 [2] on the device: (total_norm, clip_coef = min(1, max_norm / (total_norm + 1e-6))).  The gradients are
    not touched; nothing is read on the host."""
    lib = _lib.load()
    segs = _optim_table(segs, T, "grad_norm")
    dev, role = segs.device, "grad_norm: "
    out2 = _buf((2,), torch.float32, dev, role + "out2")
    with torch.cuda.device(dev):
        ws = _buf(max(lib.gnnrag_optim_workspace_bytes(n_chunks), 16), torch.uint8, dev, role + "workspace")
        _lib.check(lib.gnnrag_grad_norm(segs.data_ptr(), T, n_chunks, float(max_norm), out2.data_ptr(), ws.data_ptr(),
                                        ws.numel(), _stream()), "gnnrag_grad_norm")
    return out2


def adam_step(segs: torch.Tensor, T: int, n_chunks: int, clip_coef: Optional[torch.Tensor] = None) -> None:
    """One ``torch.optim.Adam`` step over every tensor of the table in one launch (``gnnrag_adam_step``): p, m and v are
    updated in place, g is read and NOT rewritten.  clip_coef: a device float tensor whose first element scales every
    gradient as it is read (``grad_norm(...)[1:]``), None for no clipping."""
    lib = _lib.load()
    segs = _optim_table(segs, T, "adam_step")
    if clip_coef is not None:
        clip_coef = _chk(clip_coef, "clip_coef")
        if clip_coef.numel() < 1 or clip_coef.device != segs.device:
            raise ValueError("adam_step: clip_coef must hold one float on the table's device")
    with torch.cuda.device(segs.device):
        _lib.check(lib.gnnrag_adam_step(segs.data_ptr(), T, n_chunks, _ptr(clip_coef), _stream()), "gnnrag_adam_step")


MAX_INS = 8                                     # GNNRAG_MAX_INS (include/gnnrag.h)


def instructions_supported(T: int, D: int, n_steps: int) -> bool:
    """Whether ``gnnrag_instructions`` takes the shape (the header's LDS budget: one question's working set in 160 KB)."""
    return (T > 0 and D > 0 and 0 < n_steps <= MAX_INS and
            4 * ((T * D + 3) // 4 * 4 + (n_steps + 2) * D + T) <= 160 * 1024)


def instructions(hidden, node, mask, W_q, b_q, W_cq, b_cq, w_ca, b_ca, r_in=None):
    """``BaseInstruction.get_instruction`` (base_encoder.py:82-101) for ``len(W_q)`` chained steps in one launch
    (``gnnrag_instructions``): hidden [B,T,D], node [B,D], mask [B,T], ``W_q`` / ``b_q`` LISTS of the steps'
    ``question_linear`` weights [D,D] and biases [D], W_cq [D,4D], b_cq [D], w_ca [D] (or ``ca_linear.weight`` [1,D]),
    b_ca [1], r_in [B,D] or None (zeros).  Returns (ins [n,B,D], attn [n,B,T]).  A shape outside the library's budget
    raises ``GnnragError`` (GNNRAG_E_UNSUPPORTED)."""
    lib = _lib.load()
    hidden = _chk(hidden, "hidden")
    if hidden.dim() != 3:
        raise ValueError("hidden must be [B,T,D]")
    B, T, D = hidden.shape
    n = len(W_q)
    if len(b_q) != n:
        raise ValueError("instructions: W_q and b_q must be lists of the same length")
    node = _chk(node, "node", shape=(B, D))
    mask = _chk(mask, "mask", shape=(B, T))
    W_q = [_chk(w.detach(), "W_q[%d]" % i, shape=(D, D)) for i, w in enumerate(W_q)]
    b_q = [_chk(v.detach(), "b_q[%d]" % i, shape=(D,)) for i, v in enumerate(b_q)]
    W_cq = _chk(W_cq.detach(), "W_cq", shape=(D, 4 * D))
    b_cq = _chk(b_cq.detach(), "b_cq", shape=(D,))
    w_ca = _chk(w_ca.detach().reshape(-1), "w_ca", shape=(D,))
    b_ca = _chk(b_ca.detach().reshape(-1), "b_ca", shape=(1,))
    r_in = None if r_in is None else _chk(r_in, "r_in", shape=(B, D))
    dev = hidden.device
    ins = _buf((max(n, 1), B, D), torch.float32, dev, "instructions: ins_out")
    attn = _buf((max(n, 1), B, T), torch.float32, dev, "instructions: attn_out")
    Wp = (C.c_void_p * max(n, 1))(*[w.data_ptr() for w in W_q])
    bp = (C.c_void_p * max(n, 1))(*[v.data_ptr() for v in b_q])
    with torch.cuda.device(dev):
        _lib.check(lib.gnnrag_instructions(hidden.data_ptr(), node.data_ptr(), mask.data_ptr(), _ptr(r_in), Wp, bp,
                                           W_cq.data_ptr(), b_cq.data_ptr(), w_ca.data_ptr(), b_ca.data_ptr(), B, T, D, n,
                                           ins.data_ptr(), attn.data_ptr(), _stream()), "gnnrag_instructions")
    return ins, attn


def instructions_backward_supported(T: int, D: int, n_steps: int) -> bool:
    """Whether ``gnnrag_instructions_train`` / ``gnnrag_instructions_backward`` take the shape (the header's LDS budgets;
    every T <= 64 with D <= 256 at 8 steps fits)."""
    return (instructions_supported(T, D, n_steps) and T * D <= 40960 and
            4 * ((T * D + 3) // 4 * 4 + 12 * D + 3 * T) <= 160 * 1024)


def _ins_args(hidden, node, W_q, W_cq, w_ca, r_in, drop_node, drop_cat, drop_tok):
    hidden = _chk(hidden, "hidden")
    if hidden.dim() != 3:
        raise ValueError("hidden must be [B,T,D]")
    B, T, D = hidden.shape
    n = len(W_q)
    node = _chk(node, "node", shape=(B, D))
    W_q = [_chk(w.detach(), "W_q[%d]" % i, shape=(D, D)) for i, w in enumerate(W_q)]
    W_cq = _chk(W_cq.detach(), "W_cq", shape=(D, 4 * D))
    w_ca = _chk(w_ca.detach().reshape(-1), "w_ca", shape=(D,))
    r_in = None if r_in is None else _chk(r_in, "r_in", shape=(B, D))
    drop_node = None if drop_node is None else _chk(drop_node, "drop_node", shape=(n, B, D))
    drop_cat = None if drop_cat is None else _chk(drop_cat, "drop_cat", shape=(n, B, 4 * D))
    drop_tok = None if drop_tok is None else _chk(drop_tok, "drop_tok", shape=(n, B, T, D))
    return hidden, node, W_q, W_cq, w_ca, r_in, drop_node, drop_cat, drop_tok, (B, T, D, n)


def instructions_train(hidden, node, mask, W_q, b_q, W_cq, b_cq, w_ca, b_ca, r_in=None, drop_node=None, drop_cat=None,
                       drop_tok=None):
    """:func:`instructions` for training (``gnnrag_instructions_train``): the same kernel, plus the three dropout
    multipliers of ``linear_drop`` - drop_node [n,B,D], drop_cat [n,B,4D], drop_tok [n,B,T,D], values 0 or 1/(1-p), None =
    ones - and the reserve (q_s and cq of every step, a uint8 tensor of ``gnnrag_instructions_reserve_bytes``) that
    :func:`instructions_backward` reads.  Without multipliers ins / attn are the bits of :func:`instructions`.  The reserve
    is allocated per call and returned: it belongs to this forward.  Returns (ins [n,B,D], attn [n,B,T], reserve)."""
    lib = _lib.load()
    hidden, node, W_q, W_cq, w_ca, r_in, drop_node, drop_cat, drop_tok, (B, T, D, n) = _ins_args(
        hidden, node, W_q, W_cq, w_ca, r_in, drop_node, drop_cat, drop_tok)
    if len(b_q) != n:
        raise ValueError("instructions_train: W_q and b_q must be lists of the same length")
    mask = _chk(mask, "mask", shape=(B, T))
    b_q = [_chk(v.detach(), "b_q[%d]" % i, shape=(D,)) for i, v in enumerate(b_q)]
    b_cq = _chk(b_cq.detach(), "b_cq", shape=(D,))
    b_ca = _chk(b_ca.detach().reshape(-1), "b_ca", shape=(1,))
    dev = hidden.device
    ins = _buf((max(n, 1), B, D), torch.float32, dev, "instructions_train: ins_out")
    attn = _buf((max(n, 1), B, T), torch.float32, dev, "instructions_train: attn_out")
    reserve = _buf(lib.gnnrag_instructions_reserve_bytes(B, T, D, n), torch.uint8, dev, "instructions_train: reserve")
    Wp = (C.c_void_p * max(n, 1))(*[w.data_ptr() for w in W_q])
    bp = (C.c_void_p * max(n, 1))(*[v.data_ptr() for v in b_q])
    with torch.cuda.device(dev):
        _lib.check(lib.gnnrag_instructions_train(hidden.data_ptr(), node.data_ptr(), mask.data_ptr(), _ptr(r_in), Wp, bp,
                                                 W_cq.data_ptr(), b_cq.data_ptr(), w_ca.data_ptr(), b_ca.data_ptr(),
                                                 _ptr(drop_node), _ptr(drop_cat), _ptr(drop_tok), B, T, D, n,
                                                 ins.data_ptr(), attn.data_ptr(), reserve.data_ptr(), reserve.numel(),
                                                 _stream()), "gnnrag_instructions_train")
    return ins, attn, reserve


INS_GRADS = ("dhidden", "dnode", "dr_in", "dW_q", "db_q", "dW_cq", "db_cq", "dw_ca", "db_ca")


def instructions_backward(hidden, node, W_q, W_cq, w_ca, ins, attn, reserve, g_ins=None, g_attn=None, r_in=None,
                          drop_node=None, drop_cat=None, drop_tok=None, need=None):
    """Backward of :func:`instructions_train` (``gnnrag_instructions_backward``): hidden, node, the weights, r_in (None =
    zeros) and the multipliers as given to the forward, ins / attn / reserve as it returned them, g_ins [n,B,D] /
    g_attn [n,B,T] the incoming gradients (None = zeros).  ``need``: a dict over ``INS_GRADS`` of what is wanted (None: all; ``dW_q`` /
    ``db_q`` take one bool or a list with one per step).  Returns a dict over ``INS_GRADS``: dhidden
    [B,T,D], dnode [B,D], dr_in [B,D], dW_q / db_q lists per step, dW_cq [D,4D], db_cq [D], dw_ca [D], db_ca [1] (exactly
    zero); an output that is not wanted is None and is not computed.  One fixed summation order: the same bits every time."""
    lib = _lib.load()
    hidden, node, W_q, W_cq, w_ca, r_in, drop_node, drop_cat, drop_tok, (B, T, D, n) = _ins_args(
        hidden, node, W_q, W_cq, w_ca, r_in, drop_node, drop_cat, drop_tok)
    ins = _chk(ins, "ins", shape=(n, B, D))
    attn = _chk(attn, "attn", shape=(n, B, T))
    reserve = _chk(reserve, "reserve", dtype=torch.uint8)
    g_ins = None if g_ins is None else _chk(g_ins, "g_ins", shape=(n, B, D))
    g_attn = None if g_attn is None else _chk(g_attn, "g_attn", shape=(n, B, T))
    need = {k: True for k in INS_GRADS} if need is None else need

    def per_step(k):
        v = need.get(k)
        return [bool(x) for x in v] if isinstance(v, (list, tuple)) else [bool(v)] * n

    dev = hidden.device
    role = "instructions_backward: "
    shapes = {"dhidden": (B, T, D), "dnode": (B, D), "dr_in": (B, D), "dW_cq": (D, 4 * D), "db_cq": (D,), "dw_ca": (D,),
              "db_ca": (1,)}
    out = {k: (_buf(shp, torch.float32, dev, role + k) if need.get(k) else None) for k, shp in shapes.items()}
    out["dW_q"] = [_buf((D, D), torch.float32, dev, role + "dW_q") if w else None for w in per_step("dW_q")]
    out["db_q"] = [_buf((D,), torch.float32, dev, role + "db_q") if w else None for w in per_step("db_q")]
    Wp = (C.c_void_p * n)(*[w.data_ptr() for w in W_q])
    dWp = (C.c_void_p * n)(*[_ptr(t) for t in out["dW_q"]])
    dbp = (C.c_void_p * n)(*[_ptr(t) for t in out["db_q"]])
    with torch.cuda.device(dev):
        # the size depends on the CURRENT device's CU count (gnnrag_gemm_tn inside): query it on hidden's device
        ws = _buf(max(lib.gnnrag_instructions_backward_workspace_bytes(B, T, D, n), 16), torch.uint8, dev,
                  role + "workspace")
        _lib.check(lib.gnnrag_instructions_backward(
            hidden.data_ptr(), node.data_ptr(), _ptr(r_in), Wp, W_cq.data_ptr(), w_ca.data_ptr(), _ptr(drop_node),
            _ptr(drop_cat), _ptr(drop_tok), ins.data_ptr(), attn.data_ptr(), reserve.data_ptr(), reserve.numel(),
            _ptr(g_ins), _ptr(g_attn), _ptr(out["dhidden"]), _ptr(out["dnode"]), _ptr(out["dr_in"]), dWp, dbp,
            _ptr(out["dW_cq"]), _ptr(out["db_cq"]), _ptr(out["dw_ca"]), _ptr(out["db_ca"]), B, T, D, n, ws.data_ptr(),
            ws.numel(), _stream()), "gnnrag_instructions_backward")
    return out


BERT_MAX_T = 128                                # keys of one question: two per lane (csrc/bert_encoder.hip)
BERT_LAYER_FIELDS = tuple(n for n, _ in _lib.BertLayer._fields_)


def bert_encode_supported(T: int, H: int, heads: int, I: int, max_pos: int, pad_id: Optional[int] = None) -> bool:
    """Whether ``gnnrag_bert_encode`` / ``gnnrag_bert_encode_ex`` takes the shape (the header's rules).  ``pad_id``: the
    padding id of an encoder whose positions come from the ids (RoBERTa, MPNet): a full row reaches position
    ``T + pad_id``, which must be a row of the position table."""
    if pad_id is not None and (pad_id < 0 or T + pad_id > max_pos - 1):
        return False
    return (0 < T <= min(BERT_MAX_T, max_pos) and H > 0 and I > 0 and heads > 0 and H % heads == 0 and H % 4 == 0 and
            H // heads in (32, 64))


def _bert_pad_id(pad_id) -> int:
    if pad_id is None:
        return -1
    if int(pad_id) < 0:
        raise ValueError("pad_id must be None (positions 0 .. T-1) or >= 0")
    return int(pad_id)


def bert_attention(qkv: torch.Tensor, B: int, T: int, heads: int, dh: int,
                   rel_bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``gnnrag_bert_attention``: qkv [B*T, 3*heads*dh] (query, key, value blocks of a row in that order) ->
    ctx [B*T, heads*dh] = softmax(q k^T / sqrt(dh)) v per (question, head), no mask.  ``rel_bias`` [heads, 2T-1]
    (``gnnrag_bert_attention_bias``): ``rel_bias[h, j - i + T - 1]`` is added to the scaled score of query i and key j."""
    lib = _lib.load()
    H = heads * dh
    qkv = _chk(qkv, "qkv", shape=(B * T, 3 * H))
    if rel_bias is not None:
        rel_bias = _chk(rel_bias.detach(), "rel_bias", shape=(heads, 2 * T - 1))
    ctx = _buf((B * T, H), torch.float32, qkv.device, "bert_attention: ctx")
    with torch.cuda.device(qkv.device):
        if rel_bias is None:
            _lib.check(lib.gnnrag_bert_attention(qkv.data_ptr(), B, T, heads, dh, ctx.data_ptr(), _stream()),
                       "gnnrag_bert_attention")
        else:
            _lib.check(lib.gnnrag_bert_attention_bias(qkv.data_ptr(), B, T, heads, dh, rel_bias.data_ptr(), ctx.data_ptr(),
                                                      _stream()), "gnnrag_bert_attention_bias")
    return ctx


def _keep_scale(scale: float, what: str) -> float:
    s = float(scale)
    if not (s > 0.0 and s != float("inf")):
        raise ValueError("%s must be finite and > 0" % what)
    return s


def bert_keep_shapes(L: int, B: int, T: int, H: int, heads: int):
    """The shapes of the two keep buffers of ``bert_encode_train``: ``keep_hidden`` (1 + 2L, B*T, H) - plane 0 the
    embedding output, plane 1 + 2l layer l's attention output projection, plane 2 + 2l its FFN output projection - and
    ``keep_att`` (L, B, heads, T, T) (query row, key column); uint8, != 0 keeps.  Their sizes are the library's
    ``gnnrag_bert_keep_hidden_bytes`` / ``gnnrag_bert_keep_att_bytes``."""
    return (1 + 2 * L, B * T, H), (L, B, heads, T, T)


def bert_attention_drop(qkv: torch.Tensor, B: int, T: int, heads: int, dh: int, keep: torch.Tensor, scale: float,
                        rel_bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``gnnrag_bert_attention_drop``: ``bert_attention`` with dropout on the probabilities.  ``keep`` [B, heads, T, T]
    uint8 (query row, key column): behind the softmax the probability of key j is multiplied by ``scale`` where the byte is
    not 0 and by 0 elsewhere; the row is not renormalised (as transformers drops them)."""
    lib = _lib.load()
    H = heads * dh
    qkv = _chk(qkv, "qkv", shape=(B * T, 3 * H))
    keep = _chk(keep, "keep", dtype=torch.uint8, shape=(B, heads, T, T))
    if rel_bias is not None:
        rel_bias = _chk(rel_bias.detach(), "rel_bias", shape=(heads, 2 * T - 1))
    ctx = _buf((B * T, H), torch.float32, qkv.device, "bert_attention_drop: ctx")
    with torch.cuda.device(qkv.device):
        _lib.check(lib.gnnrag_bert_attention_drop(qkv.data_ptr(), B, T, heads, dh, _ptr(rel_bias), keep.data_ptr(),
                                                  _keep_scale(scale, "scale"), ctx.data_ptr(), _stream()),
                   "gnnrag_bert_attention_drop")
    return ctx


def bert_encode(ids, word_emb, pos_emb, type_emb, ln_g, ln_b, eps: float, layers, heads: int, I: Optional[int] = None,
                math: Optional[int] = None, *, pad_id: Optional[int] = None,
                rel_bias: Optional[torch.Tensor] = None, splitk: bool = False) -> torch.Tensor:
    """``gnnrag_bert_encode``: ids [B,T] int64 -> the last hidden state [B,T,H] of a BERT-class encoder (no mask, no
    pooler).  ``layers``: a list of dicts with the keys ``BERT_LAYER_FIELDS`` (W_qkv [3H,H] the query / key / value weights
    stacked, b_qkv [3H], W_o, b_o, ln1_g, ln1_b, W_i [I,H], b_i, W_f [H,I], b_f, ln2_g, ln2_b); an empty list returns the
    embedding LayerNorm (``I`` then sizes nothing and defaults to 4 H).  A shape outside the library's set raises
    ``GnnragError`` (GNNRAG_E_UNSUPPORTED).

    ``type_emb=None`` (no token-type term), ``pad_id`` (positions from the ids, as RoBERTa and MPNet count them) and
    ``rel_bias`` [heads, 2T-1] (MPNet's relative attention bias, every layer) go through ``gnnrag_bert_encode_ex``; with
    the defaults the call is the one it has always been.

    ``splitk=True`` is ``gnnrag_bert_encode_splitk``: the same encoder with the four dense products of a layer on the
    split-K linear (``linear_splitk``, its own ``splits`` rule) and the GELU and LayerNorms in its reduce - made for the
    12 .. 20 rows of one question; exact fp32 whatever ``math`` says.  Not the bits of the default call: another summation
    order."""
    return _bert_encode("bert_encode", None, ids, word_emb, pos_emb, type_emb, ln_g, ln_b, eps, layers, heads, I, math,
                        pad_id, rel_bias, splitk=bool(splitk))


def bert_encode_train(ids, word_emb, pos_emb, type_emb, ln_g, ln_b, eps: float, layers, heads: int,
                      I: Optional[int] = None, math: Optional[int] = None, *, pad_id: Optional[int] = None,
                      rel_bias: Optional[torch.Tensor] = None, keep_hidden: Optional[torch.Tensor] = None,
                      scale_hidden: float = 1.0, keep_att: Optional[torch.Tensor] = None,
                      scale_att: float = 1.0) -> torch.Tensor:
    """``gnnrag_bert_encode_train``: ``bert_encode`` as a module in training mode runs it - forward only, the encoder is
    frozen.  ``keep_hidden`` / ``keep_att``: uint8 tensors of the shapes of ``bert_keep_shapes`` (!= 0 keeps; the caller
    draws them), multiplied in as ``scale_*`` (1 / (1 - p)) at transformers' four dropout sites inside the launches that
    produce the values.  ``None`` leaves that site as in inference; both ``None`` gives the bits of ``bert_encode``."""
    return _bert_encode("bert_encode_train", (keep_hidden, scale_hidden, keep_att, scale_att), ids, word_emb, pos_emb,
                        type_emb, ln_g, ln_b, eps, layers, heads, I, math, pad_id, rel_bias)


def _bert_layer_shapes(H: int, I: int):
    return {"W_qkv": (3 * H, H), "b_qkv": (3 * H,), "W_o": (H, H), "b_o": (H,), "ln1_g": (H,), "ln1_b": (H,),
            "W_i": (I, H), "b_i": (I,), "W_f": (H, I), "b_f": (H,), "ln2_g": (H,), "ln2_b": (H,)}


def _bert_layer_array(layers, H: int, I: int):
    """The host array of ``gnnrag_bert_layer`` structs and the tensors it points to (kept alive by the caller)."""
    shapes, keep, arr = _bert_layer_shapes(H, I), [], (_lib.BertLayer * max(len(layers), 1))()
    for l, layer in enumerate(layers):
        for name in BERT_LAYER_FIELDS:
            t = _chk(layer[name].detach(), "layers[%d].%s" % (l, name), shape=shapes[name])
            keep.append(t)
            setattr(arr[l], name, t.data_ptr())
    return arr, keep


def _bert_keep_args(L, B, T, H, heads, keep_hidden, scale_hidden, keep_att, scale_att):
    """The two keep buffers against the shapes of ``bert_keep_shapes``, and the scales of those that are given (the scale
    of a mask that is None goes on unchecked: the library does not read it)."""
    shape_hidden, shape_att = bert_keep_shapes(L, B, T, H, heads)
    if keep_hidden is not None:
        keep_hidden = _chk(keep_hidden, "keep_hidden", dtype=torch.uint8, shape=shape_hidden)
        scale_hidden = _keep_scale(scale_hidden, "scale_hidden")
    if keep_att is not None:
        keep_att = _chk(keep_att, "keep_att", dtype=torch.uint8, shape=shape_att)
        scale_att = _keep_scale(scale_att, "scale_att")
    return keep_hidden, float(scale_hidden), keep_att, float(scale_att)


def _bert_encode(role, drop, ids, word_emb, pos_emb, type_emb, ln_g, ln_b, eps, layers, heads, I, math, pad_id, rel_bias,
                 splitk=False):
    """The shared body of ``bert_encode`` (``drop`` None) and ``bert_encode_train`` (``drop``: the two masks and scales):
    one argument list, the entry point chosen by name."""
    lib = _lib.load()
    ids = _chk(ids, "ids", dtype=torch.int64)
    if ids.dim() != 2:
        raise ValueError("ids must be [B,T]")
    B, T = ids.shape
    word_emb = _chk(word_emb.detach(), "word_emb")
    vocab, H = word_emb.shape
    pos_emb = _chk(pos_emb.detach(), "pos_emb")
    if pos_emb.dim() != 2 or pos_emb.shape[1] != H:
        raise ValueError("pos_emb must be [max_pos,H]")
    if type_emb is not None:
        type_emb = _chk(type_emb.detach(), "type_emb")
        if type_emb.dim() != 2 or type_emb.shape[1] != H or type_emb.shape[0] < 1:
            raise ValueError("type_emb must be [>=1,H]")
    if rel_bias is not None:
        rel_bias = _chk(rel_bias.detach(), "rel_bias", shape=(heads, 2 * T - 1))
    pad = _bert_pad_id(pad_id)
    ln_g, ln_b = _chk(ln_g.detach(), "ln_g", shape=(H,)), _chk(ln_b.detach(), "ln_b", shape=(H,))
    L = len(layers)
    if L:
        I = int(layers[0]["W_i"].shape[0])
    elif I is None:
        I = 4 * H
    arr, keep = _bert_layer_array(layers, H, I)
    dev = ids.device
    if drop is not None:
        entry, drop = "gnnrag_bert_encode_train", _bert_keep_args(L, B, T, H, heads, *drop)
    elif splitk:
        entry = "gnnrag_bert_encode_splitk"
    elif type_emb is not None and pad < 0 and rel_bias is None:
        entry = "gnnrag_bert_encode"            # the call it has always been: it has no pad_id and no rel_bias argument
    else:
        entry = "gnnrag_bert_encode_ex"
    out = _buf((B, T, H), torch.float32, dev, role + ": out")
    nws = int((lib.gnnrag_bert_splitk_workspace_bytes if splitk else lib.gnnrag_bert_workspace_bytes)(B, T, H, I)) if L else 0
    ws = _buf((max(nws, 1),), torch.uint8, dev, role + ": workspace")
    with torch.cuda.device(dev):
        args = [ids.data_ptr(), word_emb.data_ptr(), vocab, pos_emb.data_ptr(), pos_emb.shape[0], _ptr(type_emb)]
        if entry != "gnnrag_bert_encode":
            args += [pad, _ptr(rel_bias)]
        args += [ln_g.data_ptr(), ln_b.data_ptr(), float(eps), L, arr, B, T, H, heads, I]
        if drop is not None:
            keep_hidden, scale_hidden, keep_att, scale_att = drop
            args += [_ptr(keep_hidden), scale_hidden, _ptr(keep_att), scale_att]
        args += [out.data_ptr(), ws.data_ptr(), nws if splitk else ws.numel(), _math(math), _stream()]
        _lib.check(getattr(lib, entry)(*args), entry)
    return out


BERT_GRAD_FIELDS = tuple(n for n, _ in _lib.BertLayerGrads._fields_)


def bert_layers_backward_supported(T: int, H: int, heads: int, I: int) -> bool:
    """Whether ``gnnrag_bert_layers_forward_save`` / ``gnnrag_bert_layers_backward`` take the shape (the header's rules:
    those of the attention kernels, and ``H % 4 == 0``, ``I % 4 == 0`` for the weight-gradient products)."""
    return (0 < T <= BERT_MAX_T and H > 0 and I > 0 and heads > 0 and H % heads == 0 and H % 4 == 0 and I % 4 == 0 and
            H // heads in (32, 64))


def _bert_layers_args(x, layers, heads, keep_hidden, scale_hidden, keep_att, scale_att, B, T, who):
    if x.dim() not in (2, 3):
        raise ValueError("%s must be [B*T,H] or [B,T,H]" % who)
    x = _chk(x, who, shape=(B * T, x.shape[-1]) if x.dim() == 2 else (B, T, x.shape[-1]))
    H, L = int(x.shape[-1]), len(layers)
    if L < 1:
        raise ValueError("bert layers: at least one layer")
    I = int(layers[0]["W_i"].shape[0])
    return (x, H, I, L) + _bert_keep_args(L, B, T, H, heads, keep_hidden, scale_hidden, keep_att, scale_att)


def bert_layers_forward_save(x0, layers, heads: int, eps: float, B: int, T: int, math: Optional[int] = None, *,
                             keep_hidden: Optional[torch.Tensor] = None, scale_hidden: float = 1.0,
                             keep_att: Optional[torch.Tensor] = None, scale_att: float = 1.0,
                             rel_bias: Optional[torch.Tensor] = None):
    """``gnnrag_bert_layers_forward_save``: the layers of ``bert_encode_train`` on ``x0`` [B*T, H] (or [B,T,H]) - the
    output of the embedding stage - with the same launches, so the bits of ``bert_encode_train`` for the same ``x0`` and
    masks.  ``keep_hidden`` has the (1 + 2L) planes of ``bert_keep_shapes`` (plane 0, the embedding's, is not read).
    ``rel_bias`` [heads, 2T-1] (MPNet's table, every layer) goes through ``gnnrag_bert_layers_forward_save_ex``; without it
    the call is the one it has always been.
    Returns ``(out, reserve)``: out of x0's shape and the reserve (uint8, ``gnnrag_bert_reserve_bytes``) that
    :func:`bert_layers_backward` reads; it is allocated per call and belongs to this forward."""
    lib = _lib.load()
    x0, H, I, L, keep_hidden, scale_hidden, keep_att, scale_att = _bert_layers_args(
        x0, layers, heads, keep_hidden, scale_hidden, keep_att, scale_att, B, T, "x0")
    arr, keep = _bert_layer_array(layers, H, I)
    dev = x0.device
    role = "bert_layers_forward_save: "
    out = _buf(tuple(x0.shape), torch.float32, dev, role + "out")
    reserve = _buf((max(int(lib.gnnrag_bert_reserve_bytes(L, B, T, H, I)), 1),), torch.uint8, dev, role + "reserve")
    ws = _buf((max(int(lib.gnnrag_bert_workspace_bytes(B, T, H, I)), 1),), torch.uint8, dev, role + "workspace")
    args, entry = [x0.data_ptr(), L, arr], "gnnrag_bert_layers_forward_save"
    if rel_bias is not None:
        rel_bias = _chk(rel_bias.detach(), "rel_bias", shape=(heads, 2 * T - 1))
        args, entry = args + [rel_bias.data_ptr()], entry + "_ex"
    args += [float(eps), B, T, H, heads, I, _ptr(keep_hidden), scale_hidden, _ptr(keep_att), scale_att, out.data_ptr(),
             reserve.data_ptr(), reserve.numel(), ws.data_ptr(), ws.numel(), _math(math), _stream()]
    with torch.cuda.device(dev):
        _lib.check(getattr(lib, entry)(*args), entry)
    return out, reserve


def bert_layers_backward(g_out, layers, heads: int, eps: float, B: int, T: int, reserve, *,
                         keep_hidden: Optional[torch.Tensor] = None, scale_hidden: float = 1.0,
                         keep_att: Optional[torch.Tensor] = None, scale_att: float = 1.0, need_x0: bool = True,
                         need=None, rel_bias: Optional[torch.Tensor] = None, want_rel_bias_grad: bool = False):
    """Backward of :func:`bert_layers_forward_save` (``gnnrag_bert_layers_backward``): ``g_out`` the gradient of its output,
    the layers, masks and scales as given to it, ``reserve`` as it returned it.  ``need``: per layer a dict over
    ``BERT_GRAD_FIELDS`` of what is wanted (None: everything); an unwanted gradient is None and its product is not launched.
    Returns ``(g_x0, grads)``: g_x0 of g_out's shape (None without ``need_x0``) and a list of dicts over ``BERT_GRAD_FIELDS``
    (dW_qkv [3H,H], db_qkv [3H] with the key third exactly 0, ...).  One fixed summation order: the same bits every time.
    ``rel_bias`` as given to the forward (``gnnrag_bert_layers_backward_ex``); with ``want_rel_bias_grad`` the return is
    ``(g_x0, grads, d_rel_bias)``, d_rel_bias [heads, 2T-1] the table's gradient summed over the layers."""
    lib = _lib.load()
    g_out, H, I, L, keep_hidden, scale_hidden, keep_att, scale_att = _bert_layers_args(
        g_out, layers, heads, keep_hidden, scale_hidden, keep_att, scale_att, B, T, "g_out")
    arr, keep = _bert_layer_array(layers, H, I)
    reserve = _chk(reserve, "reserve", dtype=torch.uint8)
    dev = g_out.device
    role = "bert_layers_backward: "
    shapes = _bert_layer_shapes(H, I)
    garr, grads = (_lib.BertLayerGrads * L)(), []
    for l in range(L):
        want = need[l] if need is not None else {}
        g = {}
        for name in BERT_GRAD_FIELDS:
            wanted = bool(want.get(name, False)) if need is not None else True
            g[name] = _buf(shapes[name[1:]], torch.float32, dev, role + name) if wanted else None   # dW_o: W_o's shape
            setattr(garr[l], name, _ptr(g[name]))
        grads.append(g)
    g_x0 = _buf(tuple(g_out.shape), torch.float32, dev, role + "g_x0") if need_x0 else None
    if want_rel_bias_grad and rel_bias is None:
        raise ValueError("bert_layers_backward: want_rel_bias_grad without rel_bias")
    d_rel_bias = None
    args, entry = [g_out.data_ptr(), L, arr], "gnnrag_bert_layers_backward"
    if rel_bias is not None:
        rel_bias = _chk(rel_bias.detach(), "rel_bias", shape=(heads, 2 * T - 1))
        if want_rel_bias_grad:
            d_rel_bias = _buf((heads, 2 * T - 1), torch.float32, dev, role + "d_rel_bias")
        args, entry = args + [rel_bias.data_ptr()], entry + "_ex"
    with torch.cuda.device(dev):
        # the size depends on the CURRENT device's CU count (gnnrag_gemm_tn inside): query it on g_out's device
        ws = _buf((max(int(lib.gnnrag_bert_layers_backward_workspace_bytes(B, T, H, heads, I)), 16),), torch.uint8, dev,
                  role + "workspace")
        args += [float(eps), B, T, H, heads, I, _ptr(keep_hidden), scale_hidden, _ptr(keep_att), scale_att,
                 reserve.data_ptr(), reserve.numel(), _ptr(g_x0), garr]
        if rel_bias is not None:
            args.append(_ptr(d_rel_bias))
        args += [ws.data_ptr(), ws.numel(), _stream()]
        _lib.check(getattr(lib, entry)(*args), entry)
    return (g_x0, grads, d_rel_bias) if want_rel_bias_grad else (g_x0, grads)


def bert_attention_backward(qkv: torch.Tensor, d_ctx: torch.Tensor, B: int, T: int, heads: int, dh: int,
                            keep: Optional[torch.Tensor] = None, scale: float = 1.0,
                            rel_bias: Optional[torch.Tensor] = None, want_bias_grad: bool = False):
    """``gnnrag_bert_attention_backward``: d_qkv [B*T, 3*heads*dh] from qkv, d_ctx [B*T, heads*dh] and the keep bytes
    [B, heads, T, T] of :func:`bert_attention_drop` (None: :func:`bert_attention`).  The probabilities are recomputed.
    ``rel_bias`` [heads, 2T-1] as given to the forward (``gnnrag_bert_attention_backward_bias``); with ``want_bias_grad``
    the return is ``(d_qkv, d_bias)``: :func:`bert_rel_bias_reduce` on the squares the kernel left in its workspace."""
    lib = _lib.load()
    H = heads * dh
    qkv = _chk(qkv, "qkv", shape=(B * T, 3 * H))
    d_ctx = _chk(d_ctx, "d_ctx", shape=(B * T, H))
    if keep is not None:
        keep = _chk(keep, "keep", dtype=torch.uint8, shape=(B, heads, T, T))
        scale = _keep_scale(scale, "scale")
    role = "bert_attention_backward: "
    d_qkv = _buf((B * T, 3 * H), torch.float32, qkv.device, role + "d_qkv")
    ws = _buf((max(int(lib.gnnrag_bert_attention_backward_workspace_bytes(B, T, heads)), 16),), torch.uint8, qkv.device,
              role + "workspace")
    args, entry = [qkv.data_ptr(), d_ctx.data_ptr(), B, T, heads, dh], "gnnrag_bert_attention_backward"
    if rel_bias is not None:
        rel_bias = _chk(rel_bias.detach(), "rel_bias", shape=(heads, 2 * T - 1))
        args, entry = args + [rel_bias.data_ptr()], entry + "_bias"
    args += [_ptr(keep), float(scale), d_qkv.data_ptr(), ws.data_ptr(), ws.numel(), _stream()]
    with torch.cuda.device(qkv.device):
        _lib.check(getattr(lib, entry)(*args), entry)
    if not want_bias_grad:
        return d_qkv
    sq = ws[: B * heads * 2 * T * T * 4].view(torch.float32).view(B * heads, 2, T, T)
    return d_qkv, bert_rel_bias_reduce(sq, B, T, heads)


def bert_rel_bias_reduce(sq: torch.Tensor, B: int, T: int, heads: int) -> torch.Tensor:
    """``gnnrag_bert_rel_bias_reduce``: ``d_bias[h, d + T - 1]`` = the sum over the questions b and the entries
    (i, j = i + d) of the dS squares ``sq[b * heads + h, 0]`` (``sq`` [B*heads, 2, T, T], the scratch layout of the
    attention backward), b ascending, then i ascending."""
    lib = _lib.load()
    sq = _chk(sq, "sq", shape=(B * heads, 2, T, T))
    d_bias = _buf((heads, 2 * T - 1), torch.float32, sq.device, "bert_rel_bias_reduce: d_bias")
    with torch.cuda.device(sq.device):
        _lib.check(lib.gnnrag_bert_rel_bias_reduce(sq.data_ptr(), B, T, heads, d_bias.data_ptr(), _stream()),
                   "gnnrag_bert_rel_bias_reduce")
    return d_bias


BERT_EMBED_BWD_MAX_ROWS = 65536                 # rows B T of gnnrag_bert_embed_backward (include/gnnrag.h)
BERT_EMBED_GRADS = ("d_word", "d_pos", "d_type", "d_ln_g", "d_ln_b")


def bert_embed_backward_supported(M: int, H: int) -> bool:
    """Whether ``gnnrag_bert_embed_backward`` takes ``M = B T`` rows of width ``H`` (the header's rules)."""
    return 0 < M <= BERT_EMBED_BWD_MAX_ROWS and H > 0 and H % 4 == 0


def bert_embed_scatter(dz, ids, pos, vocab: int, max_pos: int, word_pad: Optional[int] = None,
                       pos_pad: Optional[int] = None):
    """``gnnrag_bert_embed_scatter``, the table step of :func:`bert_embed_backward` alone: ``(d_word [vocab,H], d_pos
    [max_pos,H])`` from ``dz`` [M,H], ``ids`` [M] int64 and ``pos`` [M] int32 - row k the sum of the dz rows that name it in
    ascending row order, +0 where none does and at the pad rows."""
    lib = _lib.load()
    dz = _chk(dz, "dz")
    M, H = dz.shape
    ids, pos = _chk(ids, "ids", dtype=torch.int64, shape=(M,)), _chk(pos, "pos", dtype=torch.int32, shape=(M,))
    role = "bert_embed_scatter: "
    d_word = _buf((vocab, H), torch.float32, dz.device, role + "d_word")
    d_pos = _buf((max_pos, H), torch.float32, dz.device, role + "d_pos")
    with torch.cuda.device(dz.device):
        _lib.check(lib.gnnrag_bert_embed_scatter(dz.data_ptr(), ids.data_ptr(), pos.data_ptr(), M, H, int(vocab), int(max_pos),
                                                 -1 if word_pad is None else int(word_pad),
                                                 -1 if pos_pad is None else int(pos_pad), d_word.data_ptr(),
                                                 d_pos.data_ptr(), _stream()), "gnnrag_bert_embed_scatter")
    return d_word, d_pos


def _bert_embed_args(ids, H, keep, scale):
    ids = _chk(ids, "ids", dtype=torch.int64)
    if ids.dim() != 2:
        raise ValueError("ids must be [B,T]")
    B, T = ids.shape
    if keep is not None:
        keep = _chk(keep, "keep", dtype=torch.uint8, shape=(B * T, H))
        scale = _keep_scale(scale, "scale")
    return ids, int(B), int(T), keep, float(scale)


def bert_embed_forward_save(ids, word_emb, pos_emb, type_emb, ln_g, ln_b, eps: float, *, pad_id: Optional[int] = None,
                            keep: Optional[torch.Tensor] = None, scale: float = 1.0):
    """``gnnrag_bert_embed_forward_save``: the embedding stage of ``bert_encode_train`` - ids [B,T] -> ``x0`` [B,T,H] with
    that call's bits for the same tables and ``keep`` (plane 0 of its ``keep_hidden``: uint8 [B*T,H], or None) - and the
    reserve (uint8, ``gnnrag_bert_embed_reserve_bytes``) that :func:`bert_embed_backward` reads.  ``type_emb`` / ``pad_id``
    as in ``bert_encode``.  Returns ``(x0, reserve)``."""
    lib = _lib.load()
    word_emb = _chk(word_emb.detach(), "word_emb")
    vocab, H = word_emb.shape
    ids, B, T, keep, scale = _bert_embed_args(ids, H, keep, scale)
    pos_emb = _chk(pos_emb.detach(), "pos_emb")
    if pos_emb.dim() != 2 or pos_emb.shape[1] != H:
        raise ValueError("pos_emb must be [max_pos,H]")
    if type_emb is not None:
        type_emb = _chk(type_emb.detach(), "type_emb")
        if type_emb.dim() != 2 or type_emb.shape[1] != H or type_emb.shape[0] < 1:
            raise ValueError("type_emb must be [>=1,H]")
    ln_g, ln_b = _chk(ln_g.detach(), "ln_g", shape=(H,)), _chk(ln_b.detach(), "ln_b", shape=(H,))
    dev, role = ids.device, "bert_embed_forward_save: "
    out = _buf((B, T, H), torch.float32, dev, role + "out")
    reserve = _buf((max(int(lib.gnnrag_bert_embed_reserve_bytes(B, T, H)), 16),), torch.uint8, dev, role + "reserve")
    with torch.cuda.device(dev):
        _lib.check(lib.gnnrag_bert_embed_forward_save(ids.data_ptr(), word_emb.data_ptr(), vocab, pos_emb.data_ptr(),
                                                      pos_emb.shape[0], _ptr(type_emb), _bert_pad_id(pad_id),
                                                      ln_g.data_ptr(), ln_b.data_ptr(), float(eps), B, T, H, _ptr(keep),
                                                      scale, out.data_ptr(), reserve.data_ptr(), reserve.numel(),
                                                      _stream()), "gnnrag_bert_embed_forward_save")
    return out, reserve


def bert_embed_backward(g_x0, ids, reserve, ln_g, eps: float, vocab: int, max_pos: int, n_type: int = 0, *,
                        word_pad: Optional[int] = None, pos_pad: Optional[int] = None,
                        keep: Optional[torch.Tensor] = None, scale: float = 1.0, need=None):
    """Backward of :func:`bert_embed_forward_save` (``gnnrag_bert_embed_backward``): ``g_x0`` [B,T,H] (or [B*T,H]) the
    gradient of its output, ``ids``, ``keep`` and ``scale`` as given to it, ``reserve`` as it returned it.  ``word_pad`` /
    ``pos_pad``: the table row whose gradient stays zero (transformers' ``padding_idx``; None: no such row).  ``n_type``: the
    rows of the token-type table (0: the encoder has none).  ``need``: a dict over ``BERT_EMBED_GRADS`` of what is wanted
    (None: everything the encoder has); an unwanted gradient is None and is not computed.  Returns a dict over
    ``BERT_EMBED_GRADS``: d_word [vocab,H], d_pos [max_pos,H], d_type [n_type,H], d_ln_g, d_ln_b [H], every one fully
    written - a row no token names is +0 - in one fixed summation order: the same bits every time."""
    lib = _lib.load()
    H = int(g_x0.shape[-1])
    ids, B, T, keep, scale = _bert_embed_args(ids, H, keep, scale)
    g_x0 = _chk(g_x0, "g_x0", shape=(B * T, H) if g_x0.dim() == 2 else (B, T, H))
    reserve = _chk(reserve, "reserve", dtype=torch.uint8)
    ln_g = _chk(ln_g.detach(), "ln_g", shape=(H,))
    dev, role = g_x0.device, "bert_embed_backward: "
    shapes = {"d_word": (vocab, H), "d_pos": (max_pos, H), "d_type": (n_type, H), "d_ln_g": (H,), "d_ln_b": (H,)}
    out = {}
    for name in BERT_EMBED_GRADS:
        wanted = (bool(need.get(name, False)) if need is not None else True) and (name != "d_type" or n_type > 0)
        out[name] = _buf(shapes[name], torch.float32, dev, role + name) if wanted else None
    ws = _buf((max(int(lib.gnnrag_bert_embed_backward_workspace_bytes(B, T, H)), 16),), torch.uint8, dev, role + "workspace")
    with torch.cuda.device(dev):
        _lib.check(lib.gnnrag_bert_embed_backward(g_x0.data_ptr(), ids.data_ptr(), reserve.data_ptr(), reserve.numel(), B, T,
                                                  H, int(vocab), int(max_pos), int(n_type),
                                                  -1 if word_pad is None else int(word_pad),
                                                  -1 if pos_pad is None else int(pos_pad), _ptr(keep), scale,
                                                  ln_g.data_ptr(), float(eps), *[_ptr(out[n]) for n in BERT_EMBED_GRADS],
                                                  ws.data_ptr(), ws.numel(), _stream()), "gnnrag_bert_embed_backward")
    return out


def bert_ln_backward(dy: torch.Tensor, d: torch.Tensor, g: torch.Tensor, eps: float,
                     keep: Optional[torch.Tensor] = None, scale: float = 1.0, res: Optional[torch.Tensor] = None):
    """``gnnrag_bert_ln_backward``: the backward of ``LN(z) g + b`` for the rows z = d * (keep ? scale : 0) + res (``keep``
    uint8 [M,H] and ``res`` [M,H] together) or z = d (both None).  Returns ``(dz, dY, dgamma, dbeta)``: dz [M,H] the
    gradient of z (and of res), dY = dz * (keep ? scale : 0) the gradient of d (dz itself without a mask), and the two
    parameter gradients [H]."""
    lib = _lib.load()
    dy = _chk(dy, "dy")
    M, H = dy.shape
    d = _chk(d, "d", shape=(M, H))
    g = _chk(g.detach(), "g", shape=(H,))
    if (keep is None) != (res is None):
        raise ValueError("bert_ln_backward: keep and res go together")
    if keep is not None:
        keep = _chk(keep, "keep", dtype=torch.uint8, shape=(M, H))
        res = _chk(res, "res", shape=(M, H))
        scale = _keep_scale(scale, "scale")
    dev, role = dy.device, "bert_ln_backward: "
    dz = _buf((M, H), torch.float32, dev, role + "dz")
    dY = _buf((M, H), torch.float32, dev, role + "dY") if keep is not None else None
    summ = _buf((M, H), torch.float32, dev, role + "summ")
    dgamma, dbeta = _buf((H,), torch.float32, dev, role + "dgamma"), _buf((H,), torch.float32, dev, role + "dbeta")
    with torch.cuda.device(dev):
        _lib.check(lib.gnnrag_bert_ln_backward(dy.data_ptr(), d.data_ptr(), _ptr(keep), float(scale), _ptr(res), g.data_ptr(),
                                               float(eps), M, H, dz.data_ptr(), _ptr(dY), summ.data_ptr(), dgamma.data_ptr(),
                                               dbeta.data_ptr(), _stream()), "gnnrag_bert_ln_backward")
    return dz, (dz if dY is None else dY), dgamma, dbeta


def bert_gelu_backward(pre: torch.Tensor, d_act: torch.Tensor, want_act: bool = False):
    """``gnnrag_bert_gelu_backward``: ``d_pre = d_act * gelu'(pre)`` (the erf form) over any shape; with ``want_act`` also
    ``gelu(pre)``.  Returns ``(d_pre, act or None)``."""
    lib = _lib.load()
    pre = _chk(pre, "pre")
    d_act = _chk(d_act, "d_act", shape=tuple(pre.shape))
    dev, role = pre.device, "bert_gelu_backward: "
    d_pre = _buf(tuple(pre.shape), torch.float32, dev, role + "d_pre")
    act = _buf(tuple(pre.shape), torch.float32, dev, role + "act") if want_act else None
    with torch.cuda.device(dev):
        _lib.check(lib.gnnrag_bert_gelu_backward(pre.data_ptr(), d_act.data_ptr(), pre.numel(), d_pre.data_ptr(), _ptr(act),
                                                 _stream()), "gnnrag_bert_gelu_backward")
    return d_pre, act


REL_TEXT_MAX_T, REL_TEXT_MAX_K, REL_TEXT_MAX_D = 256, 4096, 4096     # GNNRAG_REL_TEXT_MAX_* (include/gnnrag.h)


def rel_text_supported(R: int, T: int, K: int, D: int) -> bool:
    """Whether ``gnnrag_rel_text_pool`` takes the shape (the header's limits)."""
    return (0 < R <= 1 << 24 and 0 < T <= REL_TEXT_MAX_T and 0 < K <= REL_TEXT_MAX_K and K % 4 == 0 and
            0 < D <= REL_TEXT_MAX_D)


def _rel_text_args(X_fwd, X_inv, W, a):
    X_fwd = _chk(X_fwd, "X_fwd")
    if X_fwd.dim() != 3:
        raise ValueError("X_fwd must be [R,T,K]")
    R, T, K = X_fwd.shape
    X_inv = None if X_inv is None else _chk(X_inv, "X_inv", shape=(R, T, K))
    W = _chk(W.detach(), "W")
    D = W.shape[0]
    W = _chk(W, "W", shape=(D, K))
    a = _chk(a.detach().reshape(-1), "a", shape=(D,))
    return X_fwd, X_inv, W, a, (R, T, K, D)


def rel_text_pool(X_fwd, X_inv, mask, W, b, a, save: bool = False):
    """``get_rel_feature`` of the relation-text branch (rearev.py:101-106, nsm.py:103-105; ``gnnrag_rel_text_pool``):
    ``AttnEncoder(question_emb(X), mask)`` for the forward and - ``X_inv`` not None - the inverse relation texts, X [R,T,K]
    the LM token states, mask [R,T] (1 = token, shared by both directions), W [D,K] / b [D] = ``question_emb``, a [D] (or
    ``attn_linear.weight`` [1,D]).  Returns (out_fwd [R,D], out_inv or None, xbar, alpha); ``save`` keeps xbar
    [n_dir,R,K] and alpha [n_dir,R,T] for :func:`rel_text_pool_backward` (else both None: xbar lives in the call's
    workspace).  A shape outside the library's limits raises ``GnnragError`` (GNNRAG_E_UNSUPPORTED)."""
    lib = _lib.load()
    X_fwd, X_inv, W, a, (R, T, K, D) = _rel_text_args(X_fwd, X_inv, W, a)
    mask = _chk(mask, "mask", shape=(R, T))
    b = _chk(b.detach(), "b", shape=(D,))
    n_dir = 1 if X_inv is None else 2
    dev = X_fwd.device
    out_fwd = _buf((R, D), torch.float32, dev, "rel_text_pool: out_fwd")
    out_inv = None if X_inv is None else _buf((R, D), torch.float32, dev, "rel_text_pool: out_inv")
    xbar = _buf((n_dir, R, K), torch.float32, dev, "rel_text_pool: xbar") if save else None
    alpha = _buf((n_dir, R, T), torch.float32, dev, "rel_text_pool: alpha") if save else None
    ws = _buf(max(lib.gnnrag_rel_text_workspace_bytes(R, T, K, D, n_dir), 16), torch.uint8, dev,
              "rel_text_pool: workspace")
    with torch.cuda.device(dev):
        _lib.check(lib.gnnrag_rel_text_pool(X_fwd.data_ptr(), _ptr(X_inv), mask.data_ptr(), W.data_ptr(), b.data_ptr(),
                                            a.data_ptr(), R, T, K, D, out_fwd.data_ptr(), _ptr(out_inv), _ptr(xbar),
                                            _ptr(alpha), ws.data_ptr(), ws.numel(), _stream()), "gnnrag_rel_text_pool")
    return out_fwd, out_inv, xbar, alpha


def rel_text_pool_backward(X_fwd, X_inv, W, a, xbar, alpha, g_fwd=None, g_inv=None, need_dW=True, need_db=True,
                           need_da=True):
    """Backward of :func:`rel_text_pool` (``gnnrag_rel_text_pool_backward``): X, W, a as given to the forward, xbar / alpha
    as it returned them, g_fwd / g_inv [R,D] the incoming gradients (None = zeros).  Returns (dW [D,K], db [D], da [D]);
    an output that is not wanted is None and is not computed.  One fixed summation order: the same bits every time."""
    lib = _lib.load()
    X_fwd, X_inv, W, a, (R, T, K, D) = _rel_text_args(X_fwd, X_inv, W, a)
    n_dir = 1 if X_inv is None else 2
    xbar = _chk(xbar, "xbar", shape=(n_dir, R, K))
    alpha = _chk(alpha, "alpha", shape=(n_dir, R, T))
    g_fwd = None if g_fwd is None else _chk(g_fwd, "g_fwd", shape=(R, D))
    g_inv = None if g_inv is None else _chk(g_inv, "g_inv", shape=(R, D))
    dev = X_fwd.device
    dW = _buf((D, K), torch.float32, dev, "rel_text_pool_backward: dW") if need_dW else None
    db = _buf((D,), torch.float32, dev, "rel_text_pool_backward: db") if need_db else None
    da = _buf((D,), torch.float32, dev, "rel_text_pool_backward: da") if need_da else None
    with torch.cuda.device(dev):
        # the size depends on the CURRENT device's CU count (gnnrag_gemm_tn inside): query it on X's device
        ws = _buf(max(lib.gnnrag_rel_text_backward_workspace_bytes(R, T, K, D, n_dir), 16), torch.uint8, dev,
                  "rel_text_pool_backward: workspace")
        _lib.check(lib.gnnrag_rel_text_pool_backward(X_fwd.data_ptr(), _ptr(X_inv), W.data_ptr(), a.data_ptr(),
                                                     xbar.data_ptr(), alpha.data_ptr(), _ptr(g_fwd), _ptr(g_inv), R, T, K,
                                                     D, _ptr(dW), _ptr(db), _ptr(da), ws.data_ptr(), ws.numel(),
                                                     _stream()), "gnnrag_rel_text_pool_backward")
    return dW, db, da


def topp_candidates(pred_dist: torch.Tensor, eligible: torch.Tensor, ignore_prob: float, eps: float):
    """Per question: slots kept by the Evaluator's filter, sorted by probability (descending, stable), and
    how many of them the top-p cut retrieves.  Returns (slots int32 [B,N] (-1 padded), counts int32 [B,2])."""
    lib = _lib.load()
    pred_dist = _chk(pred_dist, "pred_dist")
    B, N = pred_dist.shape
    eligible = _chk(eligible, "eligible", dtype=torch.uint8, shape=(B, N))
    slots = _buf((B, N), torch.int32, pred_dist.device, "topp_candidates_ws: slots")
    cnt = _buf((B, 2), torch.int32, pred_dist.device, "topp_candidates_ws: counts")
    with torch.cuda.device(pred_dist.device):
        nws = lib.gnnrag_topp_workspace_bytes(B, N)          # > 0 for N > 16384: the survivors are sorted outside LDS
        ws = _buf(max(nws, 16), torch.uint8, pred_dist.device, "topp_candidates_ws: workspace")
        _lib.check(lib.gnnrag_topp_candidates_ws(pred_dist.data_ptr(), eligible.data_ptr(), B, N, float(ignore_prob),
                                                 float(eps), slots.data_ptr(), cnt.data_ptr(), ws.data_ptr(), ws.numel(),
                                                 _stream()), "gnnrag_topp_candidates_ws")
    return slots, cnt


class UGraph:
    """Simple undirected adjacency of a batch on the device (``gnnrag_ugraph_build``): per node its neighbours in
    ascending order, each with the winning fact of the pair (the largest fact id among the facts that join the two
    nodes).  What the reference's ``build_graph`` (``llm/src/utils/graph_utils.py:9-15``) makes with networkx, derived
    from the structure that is already resident.  Owns its memory like :class:`CsrPlan`."""

    def __init__(self, plan: "CsrPlan"):
        lib = _lib.load()
        self.B, self.N, self.F, self.device = plan.B, plan.N, plan.F, plan.device
        with torch.cuda.device(self.device):
            nbytes = lib.gnnrag_ugraph_bytes(self.F, self.B, self.N)
            sbytes = lib.gnnrag_ugraph_scratch_bytes(self.F, self.B, self.N)
            if nbytes == 0 or sbytes == 0:
                raise ValueError("batch too large for the undirected adjacency (2 F and B * N must fit int32)")
            self._mem = _buf(nbytes, torch.uint8, self.device, "ugraph_build: mem")
            scratch = _buf(sbytes, torch.uint8, self.device, "ugraph_build: scratch")
            self.c = _lib.UGraphStruct()
            _lib.check(lib.gnnrag_ugraph_build(C.byref(plan.c), self._mem.data_ptr(), self._mem.numel(),
                                               scratch.data_ptr(), scratch.numel(), C.byref(self.c), _stream()),
                       "gnnrag_ugraph_build")
            scratch.record_stream(torch.cuda.current_stream())      # nothing waited for the stream: keep the scratch
        self._plan = plan                   # a concatenated structure's parts stay alive with it

    @classmethod
    def from_plan(cls, plan: "CsrPlan") -> "UGraph":
        return cls(plan)

    def _dev_view(self, addr: int, n: int) -> torch.Tensor:
        off = int(addr) - self._mem.data_ptr()
        return self._mem[off: off + 4 * n].view(torch.int32)

    def to_host(self) -> dict:
        """(u_ptr [B*N+1], u_adj [U, 2]) copied back (tests and tools; waits for the stream)."""
        u_ptr = self._dev_view(self.c.u_ptr, self.B * self.N + 1).cpu().numpy()
        U = int(u_ptr[-1])
        u_adj = self._dev_view(self.c.u_adj, 2 * U).cpu().numpy().reshape(-1, 2) if U else np.zeros((0, 2), np.int32)
        return {"u_ptr": u_ptr, "u_adj": u_adj}


class PathBuffers:
    """Worst-case output arrays and the workspace of ``gnnrag_shortest_paths`` for one ``(B, N, limits)``."""

    def __init__(self, B, N, max_seeds, max_cands, max_paths, max_hops, device):
        lib = _lib.load()
        self.key = (int(B), int(N), int(max_seeds), int(max_cands), int(max_paths), int(max_hops), torch.device(device))
        P = B * max_seeds * max_cands
        if lib.gnnrag_paths_out_bytes(B, max_seeds, max_cands, max_paths, max_hops) == 0:
            raise ValueError("path limits out of range (positive sizes, max_hops <= 254, pairs * max_paths < 2^31)")
        nws = lib.gnnrag_paths_workspace_bytes(B, N, max_seeds, max_cands)
        if nws == 0:
            raise _lib.GnnragError("gnnrag_shortest_paths supports at most 65536 node slots per question (N = %d)" % N)
        i32 = torch.int32
        self.q_info = _buf((B, 2), i32, device, "shortest_paths: q_info")
        self.pair_info = _buf((B, max_seeds, max_cands, 2), i32, device, "shortest_paths: pair_info")
        self.path_off = _buf(P + 1, i32, device, "shortest_paths: path_off")
        self.path_nodes = _buf((P * max_paths, max_hops + 1), i32, device, "shortest_paths: path_nodes")
        self.path_facts = _buf((P * max_paths, max_hops), i32, device, "shortest_paths: path_facts")
        self.ws = _buf(nws, torch.uint8, device, "shortest_paths: workspace")


_path_buffers = {}


def shortest_paths(graph: "UGraph", seed_flag: torch.Tensor, cand_slot: torch.Tensor, cand_cnt: torch.Tensor,
                   max_seeds: int = 4, max_cands: int = 16, max_paths: int = 64, max_hops: int = 8,
                   buffers: Optional["PathBuffers"] = None) -> "PathBuffers":
    """All shortest paths seed -> candidate per question (``gnnrag_shortest_paths``; the reference's ``get_truth_paths``,
    ``llm/src/utils/graph_utils.py:37-60``).  ``cand_slot`` / ``cand_cnt`` are :func:`topp_candidates`' outputs.  Nothing
    waits for the stream; the result is the :class:`PathBuffers` holding the device arrays (one set per shape and limits
    is kept and reused when ``buffers`` is not given: copy what you keep before the next call)."""
    lib = _lib.load()
    B, N = graph.B, graph.N
    seed_flag = _chk(seed_flag, "seed_flag", dtype=torch.uint8, shape=(B, N))
    cand_slot = _chk(cand_slot, "cand_slot", dtype=torch.int32, shape=(B, N))
    cand_cnt = _chk(cand_cnt, "cand_cnt", dtype=torch.int32, shape=(B, 2))
    for name, t in (("seed_flag", seed_flag), ("cand_slot", cand_slot), ("cand_cnt", cand_cnt)):
        if t.device != graph.device:
            raise _lib.GnnragError("%s lives on %s but the graph was built on %s" % (name, t.device, graph.device))
    key = (B, N, int(max_seeds), int(max_cands), int(max_paths), int(max_hops), graph.device)
    with torch.cuda.device(graph.device):
        if buffers is None:
            buffers = _path_buffers.get(key)
            if buffers is None:
                _path_buffers.clear()               # one set at a time: the worst case is large
                buffers = _path_buffers[key] = PathBuffers(*key)
        elif buffers.key != key:
            raise ValueError("buffers were made for %s, the call needs %s" % (buffers.key, key))
        o = buffers
        _lib.check(lib.gnnrag_shortest_paths(C.byref(graph.c), seed_flag.data_ptr(), cand_slot.data_ptr(),
                                             cand_cnt.data_ptr(), max_seeds, max_cands, max_paths, max_hops,
                                             o.q_info.data_ptr(), o.pair_info.data_ptr(), o.path_off.data_ptr(),
                                             o.path_nodes.data_ptr(), o.path_facts.data_ptr(), o.ws.data_ptr(),
                                             o.ws.numel(), _stream()), "gnnrag_shortest_paths")
    return buffers


class RulePathBuffers:
    """Worst-case output arrays and the workspace of ``gnnrag_rule_paths`` for one ``(F, B, N, limits)``."""

    def __init__(self, F, B, N, max_seeds, max_rules, max_paths, max_hops, device):
        lib = _lib.load()
        self.key = (int(F), int(B), int(N), int(max_seeds), int(max_rules), int(max_paths), int(max_hops),
                    torch.device(device))
        P = B * max_seeds * max_rules
        if lib.gnnrag_rule_paths_out_bytes(B, max_seeds, max_rules, max_paths, max_hops) == 0:
            raise ValueError("rule path limits out of range (positive sizes, max_hops <= 254, pairs * max_paths < 2^31)")
        nws = lib.gnnrag_rule_paths_workspace_bytes(F, B, N, max_rules, max_hops)
        if nws == 0:
            raise _lib.GnnragError("gnnrag_rule_paths supports at most 65536 node slots per question (N = %d)" % N)
        i32 = torch.int32
        self.q_info = _buf((B, 2), i32, device, "rule_paths: q_info")
        self.pair_info = _buf((B, max_seeds, max_rules, 2), i32, device, "rule_paths: pair_info")
        self.path_off = _buf(P + 1, i32, device, "rule_paths: path_off")
        self.path_nodes = _buf((P * max_paths, max_hops + 1), i32, device, "rule_paths: path_nodes")
        self.path_facts = _buf((P * max_paths, max_hops), i32, device, "rule_paths: path_facts")
        self.ws = _buf(nws, torch.uint8, device, "rule_paths: workspace")


_rule_path_buffers = {}


def rule_paths(graph: "UGraph", fact_rel: torch.Tensor, seed_flag: torch.Tensor, rule_rel: torch.Tensor,
               rule_len: torch.Tensor, max_seeds: int = 4, max_rules: int = 8, max_paths: int = 64, max_hops: int = 4,
               buffers: Optional["RulePathBuffers"] = None) -> "RulePathBuffers":
    """Every walk from a seed that follows a rule hop by hop (``gnnrag_rule_paths``; the reference's ``bfs_with_rule``,
    ``llm/src/utils/graph_utils.py:24-47``).  ``fact_rel`` [F] int32: the relation id of every fact of the batch tuple;
    ``rule_rel`` [B, max_rules, max_hops] / ``rule_len`` [B, max_rules] int32: the rules of every question (a length
    outside ``[1, max_hops]`` is an empty slot).  Nothing waits for the stream; the result is the
    :class:`RulePathBuffers` holding the device arrays (one set per shape and limits is kept and reused when ``buffers``
    is not given: copy what you keep before the next call)."""
    lib = _lib.load()
    B, N, F = graph.B, graph.N, graph.F
    fact_rel = _chk(fact_rel, "fact_rel", dtype=torch.int32, shape=(F,))
    seed_flag = _chk(seed_flag, "seed_flag", dtype=torch.uint8, shape=(B, N))
    rule_rel = _chk(rule_rel, "rule_rel", dtype=torch.int32, shape=(B, max_rules, max_hops))
    rule_len = _chk(rule_len, "rule_len", dtype=torch.int32, shape=(B, max_rules))
    for name, t in (("fact_rel", fact_rel), ("seed_flag", seed_flag), ("rule_rel", rule_rel), ("rule_len", rule_len)):
        if t.device != graph.device:
            raise _lib.GnnragError("%s lives on %s but the graph was built on %s" % (name, t.device, graph.device))
    key = (F, B, N, int(max_seeds), int(max_rules), int(max_paths), int(max_hops), graph.device)
    with torch.cuda.device(graph.device):
        if buffers is None:
            buffers = _rule_path_buffers.get(key)
            if buffers is None:
                _rule_path_buffers.clear()          # one set at a time: the worst case is large
                buffers = _rule_path_buffers[key] = RulePathBuffers(*key)
        elif buffers.key != key:
            raise ValueError("buffers were made for %s, the call needs %s" % (buffers.key, key))
        o = buffers
        _lib.check(lib.gnnrag_rule_paths(C.byref(graph.c), fact_rel.data_ptr(), seed_flag.data_ptr(), rule_rel.data_ptr(),
                                         rule_len.data_ptr(), max_seeds, max_rules, max_paths, max_hops,
                                         o.q_info.data_ptr(), o.pair_info.data_ptr(), o.path_off.data_ptr(),
                                         o.path_nodes.data_ptr(), o.path_facts.data_ptr(), o.ws.data_ptr(),
                                         o.ws.numel(), _stream()), "gnnrag_rule_paths")
    return buffers


def stream_copy(src: torch.Tensor, dst: torch.Tensor):
    lib = _lib.load()
    with torch.cuda.device(src.device):
        _lib.check(lib.gnnrag_stream_copy(src.data_ptr(), dst.data_ptr(), src.numel(), _stream()),
                   "gnnrag_stream_copy")
