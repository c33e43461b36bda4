"""One-sided communication: MPI_Win_* over HIP IPC (device) or shm (host).

``Win.Create(tensor, comm)`` exposes a tensor of every member; afterwards any member can
``Put`` / ``Get`` / ``Accumulate`` into any other member's tensor without the target's
participation. On HBM the data moves as one peer copy over xGMI (hipMemcpyAsync between
IPC-mapped allocations) and Accumulate is a fused read-modify-write kernel on the remote
memory; host windows are POSIX shm objects mapped by every member.
Synchronisation: ``Fence`` (active target, collective), ``Lock``/``Unlock`` (passive target,
shm reader/writer lock per target), ``Post``/``Start``/``Complete``/``Wait`` (PSCW), ``Flush``.
Reference: the generated Win_* / Put / Get / Accumulate wrappers (mpifuncs.c:9,1131,1656,
2322-2493); the reference never uses them, SURVEY §7.1 lists them as Tier 2.
"""
from __future__ import annotations

import ctypes
import weakref
from typing import Optional

import numpy as np
import torch

from . import datatypes as _dt
from . import runtime as _rt
from ._ext import native

LOCK_EXCLUSIVE, LOCK_SHARED = 234, 235
MODE_NOCHECK = 1024

_open = weakref.WeakSet()
_next_id = [1 << 30]


def _close_all():
    for w in list(_open):
        try:
            w.Free()
        except Exception:
            pass


def host_view(ptr: int, nbytes: int, dtype: torch.dtype) -> torch.Tensor:
    """A tensor aliasing host memory at ``ptr`` (no copy)."""
    if nbytes == 0:
        return torch.empty(0, dtype=dtype)
    buf = (ctypes.c_uint8 * nbytes).from_address(ptr)
    return torch.frombuffer(buf, dtype=dtype)


ACC_REPLACE, ACC_NO_OP = 10, 11  # csrc/kernels/kernels.h AccOp, after the ten element-wise PeerOp codes

_contig_plans = {}


def contiguous_plan(nbytes: int):
    """The one-run layout plan of `nbytes` contiguous bytes (a basic target of an accumulate)."""
    p = _contig_plans.get(nbytes)
    if p is None:
        if len(_contig_plans) >= 256:
            _contig_plans.clear()
        lens = np.array([nbytes] if nbytes > 0 else [], dtype=np.int64)
        p = _contig_plans[nbytes] = _dt.Plan((), np.zeros(len(lens), dtype=np.int64), lens)
    return p


def acc_unavailable(op) -> str:
    """Why the one-launch accumulate does not serve `op` (acc_codes gave None)."""
    if not _dt.kernel_enabled():
        return "the type_accumulate kernel is switched off (MPIT_DTYPE_KERNEL=0) or the native module did not load"
    return f"{op!r} is not a predefined reduction, REPLACE or NO_OP"


def acc_codes(what: str, op, dtype):
    """(op, dtype) codes of type_accumulate, or None when the kernel is off or `op` is not one of
    its twelve (the caller falls back or refuses). TypeError, naming both, for one of its ops on
    an element type it does not have: a float bitwise op, a type outside the seven."""
    from .comm import _PR_DTYPES, _PR_OP_CODE, NO_OP, REPLACE, _PairOp

    if not _dt.kernel_enabled():
        return None
    if isinstance(op, _PairOp):  # MAXLOC / MINLOC bound to its pair layout (comm._pair_bind)
        return _PR_OP_CODE[op.base], op.lay.code
    code = _PR_OP_CODE.get(op)
    if code is None:
        code = ACC_REPLACE if op is REPLACE else (ACC_NO_OP if op is NO_OP else None)
    if code is None:
        return None
    dc = _PR_DTYPES.get(dtype)
    if dc is None or not native().type_accumulate_supported(code, dc):
        raise TypeError(f"{what}: {op.name} is not supported on {dtype} elements")
    return code, dc


class Win:
    def __init__(self, native_win, comm, tensor: torch.Tensor, disp_unit: int, info=None):
        self._w = native_win
        self.comm = comm
        self.tensor = tensor  # the local exposed memory (a shm view for host windows)
        self.disp_unit = disp_unit
        self.info = info or {}
        self._attrs = {}
        self._name = ""
        self._epoch_targets = []
        self._errhandler = None
        _open.add(self)

    # ------------------------------------------------------------ creation
    @classmethod
    def _make(cls, tensor: Optional[torch.Tensor], nbytes: int, device: bool, comm, disp_unit: int, dtype, info=None,
              win_id: Optional[int] = None):
        eng = _rt.engine()
        if win_id is None:
            win_id = comm._agree_ctx() + (1 << 29)
        local = tensor.data_ptr() if tensor is not None and nbytes > 0 else 0
        w = native().Window(eng, int(win_id), local, int(nbytes), bool(device))
        blobs = comm.allgather_obj(bytes(w.blob()))
        w.connect(blobs, comm.world_ranks)
        if device:
            # window creation is collective: what this rank queued into the exposed memory (the
            # Allocate zero fill, the caller's writes) completes before any peer may access it
            # from its own streams, which are not ordered after ours
            torch.cuda.current_stream().synchronize()
        comm.Barrier()
        w.unlink_names()
        if device:
            exposed = tensor if tensor is not None else torch.empty(0, dtype=dtype, device=_rt.device())
        else:
            exposed = host_view(w.local_ptr, nbytes, dtype)
        return cls(w, comm, exposed, disp_unit, info)

    @classmethod
    def Create(cls, tensor: torch.Tensor, comm=None, disp_unit: Optional[int] = None, info=None) -> "Win":
        """Expose ``tensor`` (HBM: zero-copy; host: the window is a shm copy, use ``win.tensor``)."""
        from .comm import COMM_WORLD

        comm = comm or COMM_WORLD()
        if not tensor.is_contiguous():
            raise ValueError("window memory must be contiguous")
        du = disp_unit or tensor.element_size()
        return cls._make(tensor, tensor.numel() * tensor.element_size(), tensor.is_cuda, comm, du, tensor.dtype, info)

    @classmethod
    def Allocate(cls, numel: int, dtype=torch.float32, comm=None, device: Optional[bool] = None, info=None) -> "Win":
        from .comm import COMM_WORLD

        comm = comm or COMM_WORLD()
        if device is None:
            device = _rt.device() is not None
        if device:
            t = torch.zeros(numel, dtype=dtype, device=_rt.device())
            return cls._make(t, t.numel() * t.element_size(), True, comm, t.element_size(), dtype, info)
        es = torch.empty(0, dtype=dtype).element_size()
        return cls._make(None, numel * es, False, comm, es, dtype, info)

    Allocate_shared = Allocate

    # ------------------------------------------------------------ data movement
    def _stream(self):
        if _rt.device() is not None:
            return torch.cuda.current_stream().cuda_stream
        return 0

    def Put(self, origin: torch.Tensor, target_rank: int, target_disp: int = 0):
        o = origin.contiguous().reshape(-1)
        self._w.put(target_rank, target_disp * self.disp_unit, o.data_ptr(), o.numel() * o.element_size(), self._stream())
        self._keep = o

    def Get(self, origin: torch.Tensor, target_rank: int, target_disp: int = 0):
        if not origin.is_contiguous():
            raise ValueError("Get needs a contiguous origin buffer")
        self._w.get(origin.data_ptr(), target_rank, target_disp * self.disp_unit,
                    origin.numel() * origin.element_size(), self._stream())

    def _pair_acc(self, what: str, op, pairtype, origin, result, target_rank: int, target_disp: int):
        """MAXLOC / MINLOC of Accumulate / Get_accumulate: whole pairs of ``pairtype`` (None:
        interleaved pairs of the tensor's dtype), one type_accumulate launch whose element is the
        pair. ValueError, naming both, when the addresses give an item smaller than the pair."""
        from .comm import _pair_bind, _pair_unbounce

        bound, (o, r), _, bounced = _pair_bind(what, op, pairtype, (origin.contiguous(), result))
        codes = acc_codes(what, bound, o.dtype)
        if codes is None:
            raise ValueError(f"{what}: {acc_unavailable(op)}")
        ext = bound.lay.ext
        if r is not None and r.numel() != o.numel():
            raise ValueError(f"{what}: origin and result hold the same pairs")
        if not self._plan_acc(o, r, target_rank, target_disp * self.disp_unit, contiguous_plan(o.numel() * ext), codes,
                              ext):
            raise ValueError(f"{what}: {op.name} moves whole pairs of {ext} bytes; the origin, result and target "
                             "addresses give a smaller unit")
        _pair_unbounce(bounced, (result,))
        _dt.COUNTERS["rma_acc_kernel"] += 1

    def Accumulate(self, origin: torch.Tensor, target_rank: int, target_disp: int = 0, op=None, pairtype=None):
        """target = op(target, origin) element by element: every predefined reduction, REPLACE and
        NO_OP on fp32 / bf16 / fp16 / fp64 / int32 / int64 / uint8 in one type_accumulate launch
        (with MPIT_DTYPE_KERNEL=0: SUM / REPLACE on fp32 / bf16 through the axpby kernel). MAXLOC /
        MINLOC: pair by pair, ``pairtype`` as in Comm.Allreduce. Atomic
        with respect to other Accumulates on the same target (exclusive target lock); blocking."""
        from .comm import MAXLOC, MINLOC, REPLACE, SUM

        op = op or SUM
        if op is MAXLOC or op is MINLOC:
            return self._pair_acc("Accumulate", op, pairtype, origin, None, target_rank, target_disp)
        if pairtype is not None:
            raise ValueError(f"Accumulate: pairtype goes with MAXLOC / MINLOC only, not with {op!r}")
        o = origin.contiguous().reshape(-1)
        codes = acc_codes("Accumulate", op, o.dtype)
        if codes is not None and self._plan_acc(o, None, target_rank, target_disp * self.disp_unit,
                                                contiguous_plan(o.numel() * o.element_size()), codes, o.element_size()):
            _dt.COUNTERS["rma_acc_kernel"] += 1
            return
        if o.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("Accumulate supports float32 / bfloat16")
        if op is SUM:
            a, b = 1.0, 1.0
        elif op is REPLACE:
            a, b = 1.0, 0.0
        else:
            raise ValueError("Accumulate supports SUM and REPLACE")
        self._w.accumulate(target_rank, target_disp * self.disp_unit, o.data_ptr(), o.is_cuda, o.numel(),
                           o.dtype == torch.bfloat16, a, b, self._stream())
        _dt.COUNTERS["rma_acc_runs"] += 1

    def Get_accumulate(self, origin: Optional[torch.Tensor], result: torch.Tensor, target_rank: int,
                       target_disp: int = 0, op=None, pairtype=None):
        """result = target, then target = op(target, origin), element by element in one launch
        under the target's exclusive lock; complete on return. With NO_OP the origin may be None
        (an atomic Get). `result` is contiguous, of the target's element type and on the target
        window's side, like the origin. MAXLOC / MINLOC: pair by pair, ``pairtype`` as in
        Comm.Allreduce."""
        from .comm import MAXLOC, MINLOC, NO_OP, SUM

        op = op or SUM
        if not result.is_contiguous():
            raise ValueError("Get_accumulate needs a contiguous result buffer")
        if op is MAXLOC or op is MINLOC:
            if origin is None:
                raise ValueError("Get_accumulate: only NO_OP goes without an origin buffer")
            return self._pair_acc("Get_accumulate", op, pairtype, origin, result, target_rank, target_disp)
        if pairtype is not None:
            raise ValueError(f"Get_accumulate: pairtype goes with MAXLOC / MINLOC only, not with {op!r}")
        if origin is None:
            if op is not NO_OP:
                raise ValueError("Get_accumulate: only NO_OP goes without an origin buffer")
            o = None
        else:
            o = origin.contiguous().reshape(-1)
            if o.dtype != result.dtype or o.numel() != result.numel():
                raise ValueError("Get_accumulate: origin and result hold the same elements")
        codes = acc_codes("Get_accumulate", op, result.dtype)
        if codes is None:
            raise ValueError(f"Get_accumulate: {acc_unavailable(op)}")
        es = result.element_size()
        if not self._plan_acc(o, result.reshape(-1), target_rank, target_disp * self.disp_unit,
                              contiguous_plan(result.numel() * es), codes, es):
            raise ValueError("Get_accumulate: a buffer or the target is not aligned to the element size")
        _dt.COUNTERS["rma_acc_kernel"] += 1

    def Fetch_and_op(self, origin: Optional[torch.Tensor], result: torch.Tensor, target_rank: int,
                     target_disp: int = 0, op=None, pairtype=None):
        """Get_accumulate of one element (MPI_Fetch_and_op): counters, tickets, work queues. With
        MAXLOC / MINLOC the element is one pair."""
        from .comm import MAXLOC, MINLOC

        if op is MAXLOC or op is MINLOC:
            from .comm import _pair_layout

            one = _pair_layout(pairtype, result.dtype).ext
            if result.numel() * result.element_size() != one or origin is None or \
                    origin.numel() * origin.element_size() != one:
                raise ValueError("Fetch_and_op moves exactly one pair")
        elif result.numel() != 1 or (origin is not None and origin.numel() != 1):
            raise ValueError("Fetch_and_op moves exactly one element")
        self.Get_accumulate(origin, result, target_rank, target_disp, op, pairtype)

    # byte-addressed forms (the datatype-faithful Put / Get / Accumulate of mpiT.py): one
    # copy / accumulate per contiguous run of the target datatype
    def _put_bytes(self, data: torch.Tensor, target_rank: int, byte_disp: int):
        self._w.put(target_rank, int(byte_disp), data.data_ptr(), data.numel(), self._stream())
        self._keep_all = getattr(self, "_keep_all", [])
        self._keep_all.append(data)

    def _get_bytes(self, out: torch.Tensor, target_rank: int, byte_disp: int):
        self._w.get(out.data_ptr(), target_rank, int(byte_disp), out.numel() * out.element_size(), self._stream())

    # plan-addressed forms: the target datatype's whole layout (datatypes.Plan) in ONE type_copy
    # launch with the peer-mapped window as the strided side; `data` is the contiguous packed
    # stream on the window's side (HBM for a device target, host memory for a host target).
    # Complete, like every other operation, after the stream sync of Flush / Fence / Unlock.
    def _plan_copy(self, put: bool, data: torch.Tensor, target_rank: int, byte_disp: int, plan):
        if plan.total == 0:
            return
        if data.is_cuda != self._w.remote_device(target_rank) or not data.is_contiguous():
            raise ValueError("one-sided plan copy: a contiguous packed stream on the target window's side is needed")
        tab, off, table = plan.table(data.device)
        base = int(byte_disp) + off  # a single run's offset moves into the base (no table)
        unit = plan.unit(self._w.remote_ptr(target_rank) + base, data.data_ptr())
        fn = self._w.put_plan if put else self._w.get_plan
        fn(target_rank, base, list(plan.loops), tab, plan.R, plan.L, plan.per, unit, plan.lo - off, plan.hi - off,
           data.data_ptr(), self._stream())
        self._keep_all = getattr(self, "_keep_all", [])
        self._keep_all.append((data, table))

    def _acc_elems(self, data: torch.Tensor, target_rank: int, byte_disp: int, a: float, b: float):
        self._w.accumulate(target_rank, int(byte_disp), data.data_ptr(), data.is_cuda, data.numel(),
                           data.dtype == torch.bfloat16, a, b, self._stream())
        self._keep_all = getattr(self, "_keep_all", [])
        self._keep_all.append(data)
        _dt.COUNTERS["rma_acc_runs"] += 1

    # the accumulate of a whole target layout (datatypes.Plan) in ONE type_accumulate launch under
    # one exclusive target lock: `data` the origin's packed stream (None with NO_OP), `fetch` the
    # stream that receives the target's previous elements (None: no fetch), both contiguous and
    # on the window's side; codes = acc_codes(...), es the element size. Blocking: complete on
    # return. False, with nothing locked or launched, when an address makes the item smaller
    # than an element (the caller falls back or refuses).
    def _plan_acc(self, data: Optional[torch.Tensor], fetch: Optional[torch.Tensor], target_rank: int, byte_disp: int,
                  plan, codes, es: int) -> bool:
        if plan.total == 0:
            return True
        side = self._w.remote_device(target_rank)
        for t in (data, fetch):
            if t is not None and (t.is_cuda != side or not t.is_contiguous()):
                raise ValueError("one-sided accumulate: contiguous origin and result streams on the target window's "
                                 "side are needed")
        tab, off, table = plan.table((data if data is not None else fetch).device)
        base = int(byte_disp) + off
        pp = data.data_ptr() if data is not None else 0
        fp = fetch.data_ptr() if fetch is not None else 0
        unit = plan.unit(self._w.remote_ptr(target_rank) + base, pp | fp)
        if unit < es:
            return False
        self._w.accumulate_plan(target_rank, base, plan._loops, tab, plan.R, plan.L, plan.per, unit, plan.lo - off,
                                plan.hi - off, codes[0], codes[1], pp, fp, self._stream())
        return True

    def Raccumulate(self, *a, **k):
        from .comm import Request

        self.Accumulate(*a, **k)
        return Request(self.comm)

    def Rget_accumulate(self, *a, **k):
        from .comm import Request

        self.Get_accumulate(*a, **k)
        return Request(self.comm)

    def Rput(self, *a, **k):
        from .comm import Request

        self.Put(*a, **k)
        return Request(self.comm)

    def Rget(self, *a, **k):
        from .comm import Request

        self.Get(*a, **k)
        return Request(self.comm)

    # ------------------------------------------------------------ synchronisation
    def _flush(self):
        # every epoch-closing synchronisation completes the origin reads of the queued copies:
        # the origin buffers held for them (_put_bytes / _acc_elems) are released here, so a
        # Fence- or Unlock-synchronised Put loop keeps only the current epoch's origins alive
        self._w.flush(self._stream())
        self._keep_all = []

    def Flush(self, rank: Optional[int] = None):
        self._flush()

    Flush_all = Flush
    Flush_local = Flush
    Flush_local_all = Flush
    Sync = Flush

    def Fence(self, assertion: int = 0):
        self._flush()
        self.comm.Barrier()

    def Lock(self, rank: int, lock_type: int = LOCK_EXCLUSIVE, assertion: int = 0):
        self._w.lock(rank, lock_type == LOCK_EXCLUSIVE)

    def Unlock(self, rank: int):
        self._flush()
        self._w.unlock(rank)

    def Lock_all(self, assertion: int = 0):
        for r in range(self.comm.Get_size()):
            self._w.lock(r, False)

    def Unlock_all(self):
        self._flush()
        for r in range(self.comm.Get_size()):
            self._w.unlock(r)

    # PSCW: exposure epoch (Post/Wait) on the target, access epoch (Start/Complete) on the origin
    def Post(self, group, assertion: int = 0):
        z = torch.zeros(1, dtype=torch.uint8)
        self._posted = [self.comm._csend(z, self.comm._from_world(w), 31) for w in group.world_ranks]
        self._post_group = group

    def Start(self, group, assertion: int = 0):
        z = torch.zeros(1, dtype=torch.uint8)
        for w in group.world_ranks:
            self.comm._crecv(z, self.comm._from_world(w), 31).Wait()
        self._epoch_targets = list(group.world_ranks)

    def Complete(self):
        self._flush()
        z = torch.zeros(1, dtype=torch.uint8)
        for w in self._epoch_targets:
            self.comm._csend(z, self.comm._from_world(w), 32).Wait()
        self._epoch_targets = []

    def Wait(self):
        z = torch.zeros(1, dtype=torch.uint8)
        for r in getattr(self, "_posted", []):
            r.Wait()
        for w in self._post_group.world_ranks:
            self.comm._crecv(z, self.comm._from_world(w), 32).Wait()

    def Test(self) -> bool:
        self.Wait()
        return True

    # ------------------------------------------------------------ misc
    def Get_group(self):
        return self.comm.Get_group()

    def Get_attr(self, k):
        return self._attrs.get(k)

    def Set_attr(self, k, v):
        self._attrs[k] = v

    def Delete_attr(self, k):
        self._attrs.pop(k, None)

    def Get_name(self):
        return self._name

    def Set_name(self, n):
        self._name = n

    def Set_errhandler(self, eh):
        self._errhandler = eh

    def Get_errhandler(self):
        return self._errhandler

    def Call_errhandler(self, code):
        if self._errhandler:
            self._errhandler(self, code)

    def remote_ptr(self, rank: int) -> int:
        return self._w.remote_ptr(rank)

    def Free(self):
        if self._w is not None:
            try:
                self._w.flush(self._stream())
            except Exception:
                pass
            self._w = None
            self.tensor = None
