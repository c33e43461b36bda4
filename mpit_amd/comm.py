"""Communicators, requests, point-to-point and collective operations.

The reference exposes ~260 raw MPI calls taking ``(storage, count, datatype, ...)``
(mpifuncs.c, Appendix A of SURVEY.md). Here the buffer is a torch tensor (host or HBM)
and the element count / datatype are implied by it (an explicit ``count`` may shorten
it; a derived :class:`~mpit_amd.datatypes.Datatype` packs/unpacks it).

Transport is chosen by the tensor's device inside one native core:
* point-to-point: host tensors stream through the node's shm rings, HBM tensors use a
  rendezvous in which the receiver pulls the sender's buffer through HIP IPC (xGMI);
* collectives on HBM tensors go to RCCL through ``torch.distributed`` whenever every
  member owns a distinct GPU; otherwise (host tensors, or several ranks rehearsing on one
  GPU) they run as tree / ring algorithms over the point-to-point layer above;
* opt-in (``algo="window"`` / ``MPIT_ALLREDUCE=window``): all-reduce by the peer-reduce kernel
  over symmetric memory every member maps (``Comm.sym_alloc`` / ``sym_register``), a left fold
  in rank order that is bitwise identical on every rank.
"""
from __future__ import annotations

import functools
import inspect
import os
import threading
from typing import Callable, List, Optional, Sequence

import torch

from . import datatypes as _dt
from . import runtime as _rt
from ._ext import native

ANY_SOURCE = -1
ANY_TAG = -1
PROC_NULL = -2
ROOT = -3
UNDEFINED = -32766
IDENT, CONGRUENT, SIMILAR, UNEQUAL = 0, 1, 2, 3
SUCCESS = 0
ERR_TRUNCATE = 15

_COLL_OFFSET = 1 << 20  # collective traffic of a communicator uses ctx + this
# Background collectives (Comm._bg) run one at a time, in the order they were called: a ticket
# is drawn on the caller's thread and the background threads are served by ticket. (A plain
# lock lets the waiting threads in in any order, so two ranks could pair up different calls.)
_coll_cv = threading.Condition()
_coll_tickets = [0, 0]  # next ticket to hand out, ticket being served


# ============================================================================ Status / Request

class Status:
    """MPI_Status: source, tag, error, byte count, cancelled flag."""

    __slots__ = ("source", "tag", "error", "count", "cancelled", "_itemsize")

    def __init__(self, source=-1, tag=-1, error=0, count=0, cancelled=False, itemsize=1):
        self.source, self.tag, self.error, self.count, self.cancelled = source, tag, error, count, cancelled
        self._itemsize = itemsize

    @classmethod
    def _from(cls, t, itemsize=1, comm=None):
        src, tag, err, cnt, canc = t
        if comm is not None and src >= 0:
            src = comm._from_world(src)
        return cls(src, tag, err, cnt, canc, itemsize)

    def _fill(self, other: "Status"):
        for k in ("source", "tag", "error", "count", "cancelled", "_itemsize"):
            setattr(self, k, getattr(other, k))

    def Get_source(self):
        return self.source

    def Get_tag(self):
        return self.tag

    def Get_error(self):
        return self.error

    def Get_count(self, datatype=None) -> int:
        """Number of elements (bytes / element size of `datatype` or of the buffer)."""
        sz = datatype.Get_size() if datatype is not None else self._itemsize
        return self.count // max(1, sz)

    Get_elements = Get_count

    def Is_cancelled(self) -> bool:
        return self.cancelled

    def Set_cancelled(self, flag: bool):
        self.cancelled = bool(flag)

    def Set_elements(self, datatype, count: int):
        self.count = int(count) * (datatype.Get_size() if datatype is not None else self._itemsize)

    def __repr__(self):
        return f"Status(source={self.source}, tag={self.tag}, error={self.error}, count={self.count}, cancelled={self.cancelled})"


class Request:
    """A non-blocking operation. Keeps its buffers alive until completion."""

    def __init__(self, comm=None, rid: Optional[int] = None, keep=(), itemsize=1, on_done: Optional[Callable] = None,
                 work=None, thread=None, result=None, event=None):
        self.comm = comm
        self._rid = rid
        self._keep = keep
        self._itemsize = itemsize
        self._on_done = on_done
        self._work = work  # torch.distributed Work
        self._thread = thread  # background collective
        self._ev = event  # threading.Event set by the communicator's all-reduce worker
        self._status: Optional[Status] = None
        self._result = result
        self._err = None
        self._inner = None  # the request a persistent Start() took its state from
        self.persistent = None  # (callable) for *_init requests

    def _raise_err(self):
        err = self._err if self._err is not None else getattr(self._inner, "_err", None)
        if err is not None:
            raise err

    # -- completion
    def _complete(self, st: Status):
        self._status = st
        if self._on_done is not None:
            cb, self._on_done = self._on_done, None
            cb()
        self._keep = ()

    def Test(self, status: Optional[Status] = None) -> bool:
        if self._status is not None:
            if status is not None:
                status._fill(self._status)
            return True
        if self._rid is not None:
            t = _rt.engine().test(self._rid)
            if t is None:
                return False
            self._rid = None
            self._complete(Status._from(t, self._itemsize, self.comm))
        elif self._work is not None:
            if not self._work.is_completed():
                return False
            self._work.wait()
            self._work = None
            self._complete(Status(0, 0, 0, 0))
        elif self._thread is not None:
            if self._thread.is_alive():
                return False
            self._thread.join()
            self._thread = None
            self._raise_err()
            self._complete(Status(0, 0, 0, 0))
        elif self._ev is not None:
            if not self._ev.is_set():
                return False
            self._ev = None
            self._raise_err()
            self._complete(Status(0, 0, 0, 0))
        else:
            self._complete(Status())
        if status is not None:
            status._fill(self._status)
        return True

    def Wait(self, status: Optional[Status] = None) -> Status:
        if self._status is None:
            if self._rid is not None:
                t = _rt.engine().wait(self._rid)
                self._rid = None
                self._complete(Status._from(t, self._itemsize, self.comm))
            elif self._work is not None:
                self._work.wait()
                self._work = None
                self._complete(Status(0, 0, 0, 0))
            elif self._thread is not None:
                self._thread.join()
                self._thread = None
                self._raise_err()
                self._complete(Status(0, 0, 0, 0))
            elif self._ev is not None:
                self._ev.wait()
                self._ev = None
                self._raise_err()
                self._complete(Status(0, 0, 0, 0))
            else:
                self._complete(Status())
        if status is not None:
            status._fill(self._status)
        return self._status

    def Cancel(self) -> bool:
        if self._rid is not None and self._status is None:
            return bool(_rt.engine().cancel(self._rid))
        return False

    def Free(self):
        if self._rid is not None:
            try:
                _rt.engine().free_request(self._rid)
            except Exception:
                pass
            self._rid = None
        self._keep = ()

    def Get_status(self, status: Optional[Status] = None) -> bool:
        """MPI_Request_get_status: like Test but does not free the request."""
        if self._status is not None:
            if status is not None:
                status._fill(self._status)
            return True
        if self._rid is not None:
            t = _rt.engine().test(self._rid, keep=True)
            if t is None:
                return False
            if status is not None:
                status._fill(Status._from(t, self._itemsize, self.comm))
            return True
        return self.Test(status)

    def Start(self):
        """Start a persistent request (Send_init / Recv_init / ...)."""
        if self.persistent is None:
            raise RuntimeError("Start on a non-persistent request")
        r = self.persistent()
        self._rid, self._keep, self._status = r._rid, r._keep, None
        self._work, self._thread, self._on_done, self._ev = r._work, r._thread, r._on_done, r._ev
        self._err, self._inner = None, r  # (a background worker reports its error on `r`)
        r._rid = None
        return self

    @property
    def result(self):
        return self._result

    # -- multiple completion (MPI_Waitall etc.)
    @staticmethod
    def Waitall(reqs: Sequence["Request"], statuses: Optional[List[Status]] = None) -> List[Status]:
        out = [r.Wait() for r in reqs]
        if statuses is not None:
            statuses[:] = out
        return out

    @staticmethod
    def Testall(reqs: Sequence["Request"], statuses: Optional[List[Status]] = None) -> bool:
        if all(r.Test() for r in reqs):
            if statuses is not None:
                statuses[:] = [r._status for r in reqs]
            return True
        return False

    @staticmethod
    def Waitany(reqs: Sequence["Request"], status: Optional[Status] = None) -> int:
        import time

        if not reqs:
            return UNDEFINED
        while True:
            for i, r in enumerate(reqs):
                if r.Test(status):
                    return i
            time.sleep(0)

    @staticmethod
    def Testany(reqs: Sequence["Request"], status: Optional[Status] = None):
        for i, r in enumerate(reqs):
            if r.Test(status):
                return i, True
        return UNDEFINED, False

    @staticmethod
    def Waitsome(reqs: Sequence["Request"], statuses=None) -> List[int]:
        import time

        while True:
            done = Request.Testsome(reqs, statuses)
            if done:
                return done
            time.sleep(0)

    @staticmethod
    def Testsome(reqs: Sequence["Request"], statuses=None) -> List[int]:
        done = [i for i, r in enumerate(reqs) if r.Test()]
        if statuses is not None:
            statuses[:] = [reqs[i]._status for i in done]
        return done


class Grequest(Request):
    """Generalised request (MPI_Grequest_start / Grequest_complete)."""

    def __init__(self, query_fn=None, free_fn=None, cancel_fn=None, extra_state=None):
        super().__init__()
        self._done = threading.Event()
        self.query_fn, self.free_fn, self.cancel_fn, self.extra_state = query_fn, free_fn, cancel_fn, extra_state

    def Complete(self):
        self._done.set()

    def Test(self, status=None):
        if not self._done.is_set():
            return False
        st = Status(0, 0, 0, 0)
        if self.query_fn is not None:
            self.query_fn(self.extra_state, st)
        self._status = st
        if status is not None:
            status._fill(st)
        return True

    def Wait(self, status=None):
        self._done.wait()
        self.Test(status)
        return self._status

    def Cancel(self):
        if self.cancel_fn is not None:
            self.cancel_fn(self.extra_state, self._done.is_set())
        return False

    def Free(self):
        if self.free_fn is not None:
            self.free_fn(self.extra_state)


def Grequest_start(query_fn=None, free_fn=None, cancel_fn=None, extra_state=None) -> Grequest:
    return Grequest(query_fn, free_fn, cancel_fn, extra_state)


def Grequest_complete(req: Grequest):
    req.Complete()


# ============================================================================ reduction ops

class Op:
    """MPI_Op: a binary reduction on tensors (host or device)."""

    def __init__(self, fn: Callable[[torch.Tensor, torch.Tensor], torch.Tensor], commute: bool = True, name="user"):
        self.fn, self.commute, self.name = fn, commute, name

    def __call__(self, a, b):
        return self.fn(a, b)

    def Is_commutative(self) -> bool:
        return self.commute

    def Free(self):
        pass

    def __repr__(self):
        return f"Op({self.name})"


class _PairLayout:
    """How a buffer of MAXLOC / MINLOC pairs is laid out: the value dtype at byte 0, the index
    dtype at byte ``ioff``, ``ext`` bytes per pair (padding included), pointers aligned to
    ``align`` (the largest member). ``code`` is the kernels' element type (kernels.h PeerDtype);
    ``carrier`` a torch dtype of exactly ``ext`` bytes: a buffer viewed in it counts pairs, so
    every count, displacement and staging cut made on the view falls on a pair boundary."""

    __slots__ = ("name", "vdt", "idt", "ioff", "ext", "align", "code", "carrier")

    def __init__(self, name, vdt, idt, ioff, ext, align, code):
        self.name, self.vdt, self.idt, self.ioff, self.ext = name, vdt, idt, ioff, ext
        self.align, self.code = align, code
        self.carrier = {2: torch.int16, 4: torch.int32, 8: torch.int64, 16: torch.complex128}[ext]

    def members(self, t: torch.Tensor):
        """(pairs as [k, ext] bytes, values [k], indices [k]) of a contiguous buffer of whole pairs."""
        raw = t.reshape(-1).view(torch.uint8).view(-1, self.ext)
        vs = self.vdt.itemsize
        if self.vdt == self.idt and self.ioff == vs:  # interleaved, one dtype: strided views, no copy
            both = raw.view(self.vdt)
            return raw, both[:, 0], both[:, 1]
        v = raw[:, :vs].contiguous().view(self.vdt).reshape(-1)
        i = raw[:, self.ioff: self.ioff + self.idt.itemsize].contiguous().view(self.idt).reshape(-1)
        return raw, v, i


def _loc(maximum: bool, lay: Optional[_PairLayout] = None):
    """MAXLOC / MINLOC on flat buffers of k pairs, the rule of csrc/kernels/peer_ops.h
    loc_takes_b bit for bit: exactly one value NaN: that pair; otherwise the better value; on
    equal values (or both NaN) the smaller index, and a on equal or NaN indices. The result is one
    of the operand pairs, every byte of it. ``lay`` None: interleaved pairs of the tensors' dtype."""
    def f(a, b):
        ly = lay if lay is not None else _hom_layout(a.dtype)
        if a.numel() * a.element_size() % ly.ext or a.numel() * a.element_size() != b.numel() * b.element_size():
            raise ValueError(f"{'MAXLOC' if maximum else 'MINLOC'}: the operands hold whole {ly.name} pairs, "
                             "as many in each")
        ra, va, ia = ly.members(a.contiguous())
        rb, vb, ib = ly.members(b.contiguous())
        an, bn = va != va, vb != vb
        both = ~an & ~bn
        b_wins = both & ((vb > va) if maximum else (vb < va))
        a_wins = both & ((va > vb) if maximum else (va < vb))
        take_b = torch.where(an != bn, bn, b_wins | (~a_wins & (ib < ia)))
        return torch.where(take_b[:, None], rb, ra).reshape(-1).view(a.dtype).view(a.shape)

    return f


# built-in ops that act element by element (safe to apply to any chunk of a buffer)
_ELEMENTWISE_OPS = {"SUM", "PROD", "MAX", "MIN", "LAND", "BAND", "LOR", "BOR", "LXOR", "BXOR"}
SUM = Op(lambda a, b: a + b, name="SUM")
PROD = Op(lambda a, b: a * b, name="PROD")
MAX = Op(torch.maximum, name="MAX")
MIN = Op(torch.minimum, name="MIN")
LAND = Op(lambda a, b: (a.bool() & b.bool()).to(a.dtype), name="LAND")
LOR = Op(lambda a, b: (a.bool() | b.bool()).to(a.dtype), name="LOR")
LXOR = Op(lambda a, b: (a.bool() ^ b.bool()).to(a.dtype), name="LXOR")
BAND = Op(lambda a, b: a & b, name="BAND")
BOR = Op(lambda a, b: a | b, name="BOR")
BXOR = Op(lambda a, b: a ^ b, name="BXOR")
MAXLOC = Op(_loc(True), name="MAXLOC")
MINLOC = Op(_loc(False), name="MINLOC")
REPLACE = Op(lambda a, b: b, commute=False, name="REPLACE")
NO_OP = Op(lambda a, b: a, commute=False, name="NO_OP")
OP_NULL = None


def Op_create(fn: Callable, commute: bool = True) -> Op:
    """User reduction ``fn(invec, inoutvec) -> result`` (returning the combined tensor)."""
    return Op(fn, commute)


def Reduce_local(inbuf: torch.Tensor, inoutbuf: torch.Tensor, op: Op = SUM, pairtype=None):
    """MPI_Reduce_local (skipped by the reference's generator, readspec.py:73-75). ``pairtype``:
    the pair datatype of a MAXLOC / MINLOC buffer (None: interleaved pairs of the tensor's dtype)."""
    op, (a, b), _, bounced = _pair_bind("Reduce_local", op, pairtype, (inbuf, inoutbuf))
    b.copy_(op(a, b))
    _pair_unbounce(bounced, (inoutbuf,))
    return inoutbuf


# (op, dtype) codes of the peer-reduce kernel (csrc/kernels/kernels.h PeerOp / PeerDtype). The two
# pair ops come after REPLACE / NO_OP (10, 11: window.py), and run on the pair element types only.
_PR_OP_CODE = {SUM: 0, PROD: 1, MAX: 2, MIN: 3, LAND: 4, LOR: 5, LXOR: 6, BAND: 7, BOR: 8, BXOR: 9,
               MAXLOC: 12, MINLOC: 13}
_PR_DTYPES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2, torch.float64: 3, torch.int32: 4,
              torch.int64: 5, torch.uint8: 6}
_PR_PAIR = 16  # kPrPair + a _PR_DTYPES code: interleaved pairs of that dtype
_PAIR_STRUCTS = {  # datatypes._pair layouts the kernels have: name -> (value, index offset, extent, align, code)
    "MPI_FLOAT_INT": (torch.float32, 4, 8, 4, 24),
    "MPI_DOUBLE_INT": (torch.float64, 8, 16, 8, 25),
    "MPI_LONG_INT": (torch.int64, 8, 16, 8, 26),
}
_pair_layouts = {}


def _hom_layout(dtype: torch.dtype) -> _PairLayout:
    ly = _pair_layouts.get(dtype)
    if ly is None:
        code = _PR_DTYPES.get(dtype)
        if code is None:
            raise TypeError(f"MAXLOC / MINLOC: no pairs of {dtype} elements (one of {list(_PR_DTYPES)})")
        es = dtype.itemsize
        ly = _pair_layouts[dtype] = _PairLayout(f"{dtype} x 2", dtype, dtype, es, 2 * es, es, _PR_PAIR + code)
    return ly


def _pair_layout(pairtype, dtype: torch.dtype) -> _PairLayout:
    """The layout ``pairtype`` names (None: interleaved pairs of ``dtype``). TypeError, naming the
    type, for a datatype that is no pair type or whose layout the kernels do not have."""
    if pairtype is None:
        return _hom_layout(dtype)
    name = getattr(pairtype, "_name", None) or repr(pairtype)
    if name == "MPI_2INT":
        return _hom_layout(torch.int32)
    ly = _pair_layouts.get(name)
    if ly is None:
        spec = _PAIR_STRUCTS.get(name)
        tm = getattr(pairtype, "typemap", None)
        if spec is None or tm is None or len(tm) != 2 or tm[1][0] != spec[1] or pairtype.extent != spec[2]:
            raise TypeError(f"MAXLOC / MINLOC: {name} is not a supported pair datatype "
                            "(FLOAT_INT, DOUBLE_INT, LONG_INT, 2INT, or None for pairs of the tensor's dtype)")
        ly = _pair_layouts[name] = _PairLayout(name, spec[0], torch.int32, spec[1], spec[2], spec[3], spec[4])
    return ly


class _PairOp(Op):
    """MAXLOC / MINLOC bound to a pair layout, on carrier views (one element = one pair). Not
    marked commutative: a NaN float index compares with nothing, so only the left fold in rank
    order is defined, and the point-to-point paths then give the window kernels' bytes."""

    def __init__(self, base: Op, lay: _PairLayout):
        super().__init__(_loc(base is MAXLOC, lay), commute=False, name=base.name)
        self.base, self.lay = base, lay


_pair_ops = {}


def _pair_bind(what: str, op: Op, pairtype, bufs, counts=None):
    """The public reducing calls start here. Any other op: ``pairtype`` must be None, nothing
    changes. MAXLOC / MINLOC: (the op bound to its layout, the buffers as flat carrier views that
    count pairs, ``counts`` in pairs, the bounced buffers). Raises before any communication:
    ValueError for a buffer that holds no whole number of pairs, odd ``counts`` of interleaved
    elements or an address not aligned to the pair's largest member, TypeError for a pair type
    without kernels. A buffer aligned to the member but not to the pair (a float32 view from an odd
    element) has no carrier view: it is bounced through an aligned copy, ``(copy, flat buffer)`` in
    the last result, which the caller writes back where the buffer is an output
    (:func:`_pair_unbounce`)."""
    if isinstance(op, _PairOp):
        return op, bufs, counts, ()  # an inner call: bound already
    if op is not MAXLOC and op is not MINLOC:
        if pairtype is not None:
            raise ValueError(f"{what}: pairtype goes with MAXLOC / MINLOC only, not with {op!r}")
        return op, bufs, counts, ()
    first = next(b for b in bufs if b is not None)
    lay = _pair_layout(pairtype, first.dtype)
    out, bounced = [], []
    for b in bufs:
        if b is None:
            out.append(None)
            continue
        again = next((o for o, p in zip(out, bufs) if p is b), None)
        if again is not None:  # in place: one view for both
            out.append(again)
            continue
        t = _flat(b)
        if pairtype is None and t.dtype != lay.vdt:
            raise ValueError(f"{what}: {op.name} buffers of {t.dtype} and {lay.vdt} elements")
        nb = _nbytes(t)
        if nb % lay.ext:
            raise ValueError(f"{what}: {op.name} needs whole {lay.name} pairs of {lay.ext} bytes, the buffer has "
                             f"{t.numel()} elements ({nb} bytes)")
        addr = t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size()
        if addr % lay.align:
            raise ValueError(f"{what}: a buffer of {lay.name} pairs must be aligned to {lay.align} bytes")
        if addr % lay.ext:
            tmp = torch.empty(nb // lay.ext, dtype=lay.carrier, device=t.device)
            tmp.view(torch.uint8).copy_(t.view(torch.uint8))
            bounced.append((tmp, t))
            out.append(tmp)
        else:
            out.append(t.view(torch.uint8).view(lay.carrier))
    if counts is not None and pairtype is None:
        if any(int(c) % 2 for c in counts):
            raise ValueError(f"{what}: {op.name} counts of interleaved elements must be even")
        counts = [int(c) // 2 for c in counts]
    key = (op, lay.name)
    bound = _pair_ops.get(key)
    if bound is None:
        bound = _pair_ops[key] = _PairOp(op, lay)
    return bound, out, counts, bounced


def _pair_unbounce(bounced, outputs):
    """Write the aligned copies of :func:`_pair_bind` back into the caller's output buffers."""
    for tmp, t in bounced:
        if any(o is not None and o.data_ptr() == t.data_ptr() for o in outputs):
            t.view(torch.uint8).copy_(tmp.view(torch.uint8))


def _pair_call(fn):
    """A reducing method of Comm that takes ``pairtype``: with MAXLOC / MINLOC it runs on the
    carrier views of :func:`_pair_bind` and the op bound to the layout (``recvcounts`` in pairs),
    and hands the caller's own buffer back; with any other op it runs as it is."""
    names = list(inspect.signature(fn).parameters)
    i_op, i_pt = names.index("op") - 1, names.index("pairtype") - 1
    sig = inspect.signature(fn)

    @functools.wraps(fn)
    def call(self, *args, **kw):
        op = args[i_op] if len(args) > i_op else kw.get("op", SUM)
        if op is not MAXLOC and op is not MINLOC:
            if (args[i_pt] if len(args) > i_pt else kw.get("pairtype")) is not None and not isinstance(op, _PairOp):
                raise ValueError(f"{fn.__name__}: pairtype goes with MAXLOC / MINLOC only, not with {op!r}")
            return fn(self, *args, **kw)
        ba = sig.bind(self, *args, **kw)
        a = ba.arguments
        send, recv = a["sendbuf"], a.get("recvbuf")
        bound, (s2, r2), counts, bounced = _pair_bind(fn.__name__, op, a.get("pairtype"), (send, recv),
                                                      a.get("recvcounts"))
        a["op"], a["sendbuf"], a["pairtype"] = bound, s2, None
        if "recvbuf" in a:
            a["recvbuf"] = r2
        if "recvcounts" in a:
            a["recvcounts"] = counts
        out = fn(*ba.args, **ba.kwargs)
        outputs = (recv,) if recv is not None or "root" in a else (send,)  # (recvbuf None: in place, but for Reduce)
        if isinstance(out, Request):
            out._keep = (getattr(out, "_keep", None), send, recv)
            if bounced:  # (a bounced buffer completes the call here: its copy goes back before the caller looks)
                out.Wait()
                _pair_unbounce(bounced, outputs)
            return out
        _pair_unbounce(bounced, outputs)
        return recv if recv is not None and (out is r2 or out is s2) else (send if out is s2 else out)

    return call


def _pr_codes(op: Op, dtype: torch.dtype):
    """(op code, element type code) for the kernels, None where there is none."""
    if isinstance(op, _PairOp):
        return _PR_OP_CODE[op.base], op.lay.code
    return _PR_OP_CODE.get(op), _PR_DTYPES.get(dtype)


# the collectives with a window path (Comm.coll_stats keys)
_WIN_COLLS = ("reduce_scatter", "allgather", "alltoall", "bcast", "reduce", "scan", "exscan")
# the irregular collectives with a window path (Comm.vcoll_stats keys)
_WIN_VCOLLS = ("gatherv", "scatterv", "alltoallv", "alltoallw")
# what a member may find wrong with its own buffers (published in the descriptor exchange)
_VCOLL_ERRORS = {1: "a count / displacement pair lies outside its buffer",
                 2: "a tensor needs more than three loops (or has a negative stride)",
                 3: "a destination overlaps a source that is not this rank's own in-place part",
                 4: "a destination tensor has a zero or overlapping stride"}


class _SymRec:
    """A registered symmetric range: [lo, hi) byte addresses of ``tensor``, exposed by ``win``."""

    __slots__ = ("lo", "hi", "win", "tensor", "owned")

    def __init__(self, lo, hi, win, tensor, owned):
        self.lo, self.hi, self.win, self.tensor, self.owned = lo, hi, win, tensor, owned


def _rccl_op(op: Op):
    import torch.distributed as dist

    return {SUM: dist.ReduceOp.SUM, PROD: dist.ReduceOp.PRODUCT, MAX: dist.ReduceOp.MAX, MIN: dist.ReduceOp.MIN,
            BAND: dist.ReduceOp.BAND, BOR: dist.ReduceOp.BOR, BXOR: dist.ReduceOp.BXOR}.get(op)


# ============================================================================ helpers

def _flat(buf: torch.Tensor, count: Optional[int] = None) -> torch.Tensor:
    if not isinstance(buf, torch.Tensor):
        raise TypeError("buffers are torch tensors")
    if not buf.is_contiguous():
        raise ValueError("communication buffers must be contiguous")
    v = buf.reshape(-1)
    if count is not None:
        v = v[:count]
    return v


def _nbytes(t: torch.Tensor) -> int:
    return t.numel() * t.element_size()


# ============================================================================ communicator

class Comm:
    """An MPI-style communicator over a subset of the world ranks."""

    def __init__(self, ranks: Sequence[int], ctx: int, name: str = ""):
        self._ranks = list(ranks)
        self._ctx = int(ctx)
        self._name = name
        self._attrs = {}
        self._errhandler = None
        self._pg = None
        self._pg_tried = False
        me = _rt.state().rank if _rt.Initialized() else 0
        self._rank = self._ranks.index(me) if me in self._ranks else UNDEFINED
        self._w2c = {w: i for i, w in enumerate(self._ranks)}
        self.topology = None  # set by Cart_create / Graph_create
        # window all-reduce: registered symmetric memory, staging buffers, the FIFO worker
        self._sym: list = []  # _SymRec
        self._ar_stage: dict = {}  # "cuda" | "cpu" -> staging tensor (symmetric, uint8)
        self._ar_q = None
        self._ar_thread = None
        self._ar_stream = None
        self._ar_lock = threading.Lock()
        self._ar_calls = {"window": 0, "window_staged": 0, "p2p": 0, "rccl": 0}
        self._ar_off = False  # a member cannot run Window::allreduce: "window" falls back (agreed)
        self._coll_calls = {c: {"window": 0, "window_staged": 0, "fallback": 0} for c in _WIN_COLLS}
        self._vcoll_calls = {c: {"window": 0, "window_staged": 0, "fallback": 0} for c in _WIN_VCOLLS}

    # ---------------------------------------------------------------- basics
    def Get_rank(self) -> int:
        return self._rank

    def Get_size(self) -> int:
        return len(self._ranks)

    rank = property(Get_rank)
    size = property(Get_size)

    def Get_group(self):
        from .group import Group

        return Group(self._ranks)

    def Get_name(self) -> str:
        return self._name

    def Set_name(self, name: str):
        self._name = name

    def Is_inter(self) -> bool:
        return False

    def Get_remote_size(self) -> int:
        raise RuntimeError("not an inter-communicator")

    def _to_world(self, r: int) -> int:
        if r in (ANY_SOURCE, PROC_NULL):
            return r
        return self._ranks[r]

    def _from_world(self, w: int) -> int:
        return self._w2c.get(w, w)

    @property
    def world_ranks(self) -> List[int]:
        return list(self._ranks)

    # ---------------------------------------------------------------- attributes / errhandlers
    def Set_attr(self, keyval: int, value):
        self._attrs[keyval] = value

    def Get_attr(self, keyval: int):
        return self._attrs.get(keyval)

    def Delete_attr(self, keyval: int):
        self._attrs.pop(keyval, None)

    def Set_errhandler(self, eh):
        self._errhandler = eh

    def Get_errhandler(self):
        return self._errhandler

    def Call_errhandler(self, errorcode: int):
        if self._errhandler is not None:
            self._errhandler(self, errorcode)

    # ---------------------------------------------------------------- point-to-point
    def _isend(self, buf, dest, tag, ctx, sync=False, count=None, datatype=None) -> Request:
        if dest == PROC_NULL:
            return Request(self)
        if datatype is not None and not datatype.is_contiguous_basic():
            buf = datatype.pack(buf, count)
            count = None
        elif isinstance(buf, torch.Tensor) and not buf.is_contiguous():
            buf = _dt.pack_tensor(buf)  # a strided view: its elements in logical order, one launch
        t = _flat(buf, count)
        if t.is_cuda:  # the receiver pulls the bytes: what the stream is still producing must land first
            torch.cuda.current_stream(t.device).synchronize()
        rid = _rt.engine().isend(t.data_ptr(), _nbytes(t), t.is_cuda, self._to_world(dest), int(tag), ctx, sync)
        return Request(self, rid, keep=(t,), itemsize=t.element_size())

    def _irecv(self, buf, source, tag, ctx, count=None, datatype=None) -> Request:
        if source == PROC_NULL:
            r = Request(self)
            r._status = Status(PROC_NULL, ANY_TAG, 0, 0)
            return r
        if datatype is not None and not datatype.is_contiguous_basic():
            stage = datatype.staging(buf, count)
            rid = _rt.engine().irecv(stage.data_ptr(), _nbytes(stage), stage.is_cuda, self._to_world(source), int(tag), ctx)
            return Request(self, rid, keep=(stage, buf), itemsize=datatype.Get_size(),
                           on_done=lambda: datatype.unpack(stage, buf, count))
        if isinstance(buf, torch.Tensor) and not buf.is_contiguous():
            # a strided view: receive into a contiguous staging buffer that starts as the view's own
            # elements (a shorter message leaves the rest as it was) and scatter it on completion
            _dt.check_writable_layout(buf)
            stage = _dt.pack_tensor(buf)
            t = _flat(stage, count)
            if t.is_cuda:  # the sender's copy into the staging buffer must not overtake that fill
                torch.cuda.current_stream(t.device).synchronize()
            rid = _rt.engine().irecv(t.data_ptr(), _nbytes(t), t.is_cuda, self._to_world(source), int(tag), ctx)
            return Request(self, rid, keep=(stage, buf), itemsize=t.element_size(),
                           on_done=lambda: _dt.unpack_tensor(stage, buf))
        t = _flat(buf, count)
        rid = _rt.engine().irecv(t.data_ptr(), _nbytes(t), t.is_cuda, self._to_world(source), int(tag), ctx)
        return Request(self, rid, keep=(t,), itemsize=t.element_size())

    def Isend(self, buf, dest: int, tag: int = 0, count=None, datatype=None) -> Request:
        return self._isend(buf, dest, tag, self._ctx, False, count, datatype)

    def Issend(self, buf, dest: int, tag: int = 0, count=None, datatype=None) -> Request:
        return self._isend(buf, dest, tag, self._ctx, True, count, datatype)

    # MPI's buffered / ready modes: the engine never needs the user's attached buffer (eager
    # messages are copied into the shm ring, large ones wait for the receiver) and a ready
    # send is a correct standard send, so both are the standard mode
    Ibsend = Isend
    Irsend = Isend

    def Send(self, buf, dest: int, tag: int = 0, count=None, datatype=None):
        self.Isend(buf, dest, tag, count, datatype).Wait()

    Bsend = Send
    Rsend = Send

    def Ssend(self, buf, dest: int, tag: int = 0, count=None, datatype=None):
        self.Issend(buf, dest, tag, count, datatype).Wait()

    def Irecv(self, buf, source: int = ANY_SOURCE, tag: int = ANY_TAG, count=None, datatype=None) -> Request:
        return self._irecv(buf, source, tag, self._ctx, count, datatype)

    def Recv(self, buf, source: int = ANY_SOURCE, tag: int = ANY_TAG, status: Optional[Status] = None,
             count=None, datatype=None) -> Status:
        return self.Irecv(buf, source, tag, count, datatype).Wait(status)

    def Sendrecv(self, sendbuf, dest, sendtag, recvbuf, source=ANY_SOURCE, recvtag=ANY_TAG, status=None,
                 sendcount=None, sendtype=None, recvcount=None, recvtype=None) -> Status:
        rr = self.Irecv(recvbuf, source, recvtag, recvcount, recvtype)
        sr = self.Isend(sendbuf, dest, sendtag, sendcount, sendtype)
        sr.Wait()
        return rr.Wait(status)

    def Sendrecv_replace(self, buf, dest, sendtag, source=ANY_SOURCE, recvtag=ANY_TAG, status=None,
                         count=None, datatype=None) -> Status:
        tmp = buf.clone()
        return self.Sendrecv(tmp, dest, sendtag, buf, source, recvtag, status, count, datatype, count, datatype)

    def Iprobe(self, source: int = ANY_SOURCE, tag: int = ANY_TAG, status: Optional[Status] = None) -> bool:
        src = self._to_world(source) if source >= 0 else source
        t = _rt.engine().iprobe(src, int(tag), self._ctx)
        if t is None:
            return False
        if status is not None:
            status._fill(Status._from(t, 1, self))
        return True

    def Probe(self, source: int = ANY_SOURCE, tag: int = ANY_TAG, status: Optional[Status] = None) -> Status:
        src = self._to_world(source) if source >= 0 else source
        st = Status._from(_rt.engine().probe(src, int(tag), self._ctx), 1, self)
        if status is not None:
            status._fill(st)
        return st

    # persistent requests
    def Send_init(self, buf, dest, tag=0, count=None, datatype=None) -> Request:
        r = Request(self)
        r._status = Status()
        r.persistent = lambda: self.Isend(buf, dest, tag, count, datatype)
        return r

    Bsend_init = Send_init
    Rsend_init = Send_init

    def Ssend_init(self, buf, dest, tag=0, count=None, datatype=None) -> Request:
        r = Request(self)
        r._status = Status()
        r.persistent = lambda: self.Issend(buf, dest, tag, count, datatype)
        return r

    def Recv_init(self, buf, source=ANY_SOURCE, tag=ANY_TAG, count=None, datatype=None) -> Request:
        r = Request(self)
        r._status = Status()
        r.persistent = lambda: self.Irecv(buf, source, tag, count, datatype)
        return r

    # object convenience (mpiT.serialize / deserialize, init.lua:111-132)
    def send_obj(self, obj, dest: int, tag: int = 0):
        from .utils.serialize import serialize

        payload = serialize(obj)
        n = torch.tensor([payload.numel()], dtype=torch.int64)
        self.Send(n, dest, tag)
        self.Send(payload, dest, tag)

    def recv_obj(self, source: int = ANY_SOURCE, tag: int = ANY_TAG):
        from .utils.serialize import deserialize

        n = torch.zeros(1, dtype=torch.int64)
        st = self.Recv(n, source, tag)
        payload = torch.empty(int(n.item()), dtype=torch.uint8)
        self.Recv(payload, st.source, st.tag)
        return deserialize(payload)

    # ---------------------------------------------------------------- collective plumbing
    def _cctx(self) -> int:
        return self._ctx + _COLL_OFFSET

    def _csend(self, buf, dest, tag=0) -> Request:
        return self._isend(buf, dest, tag, self._cctx())

    def _crecv(self, buf, source, tag=0) -> Request:
        return self._irecv(buf, source, tag, self._cctx())

    def _use_rccl(self, t: torch.Tensor) -> bool:
        """Run this collective through torch.distributed: RCCL for HBM tensors when every
        rank owns its GPU; gloo for host tensors only when MPIT_DIST_HOST=1 (the shm
        point-to-point algorithms below are the default host path; the switch exists so
        CPU tests exercise the torch.distributed branch and its Request(work=...))."""
        if self.Get_size() == 1:
            return False
        st = _rt.state()
        if t.is_cuda:
            if st.shared_devices:
                return False
        elif os.environ.get("MPIT_DIST_HOST") != "1":
            return False
        import torch.distributed as dist

        if not dist.is_initialized():
            return False
        if self._pg is None and not self._pg_tried:
            self._pg_tried = True
            # torch.distributed only for communicators over every rank in world order (WORLD,
            # its Dup, an all-ranks Split keyed by rank): the torch group's rank order is
            # then the communicator's. Sub-communicators run on the native point-to-point
            # engine (IPC peer copies over xGMI for HBM tensors): torch's locally
            # synchronised sub-groups deadlock when two of them overlap in a rank
            # (reproduced with gloo: [0,2] then [1,2]), and communicator creation is not
            # collective over WORLD, so world-synchronised groups cannot be made either.
            if list(self._ranks) == list(range(st.world)):
                self._pg = dist.group.WORLD
        return self._pg is not None

    # ---------------------------------------------------------------- collectives
    def Barrier(self):
        if self.Get_size() == 1:
            return
        if len(self._ranks) == _rt.state().world:
            _rt.engine().barrier()
            return
        # dissemination barrier over zero-byte messages
        n, r = self.Get_size(), self.Get_rank()
        z = torch.zeros(0, dtype=torch.uint8)
        k = 1
        while k < n:
            rr = self._crecv(torch.zeros(0, dtype=torch.uint8), (r - k) % n, 7)
            self._csend(z, (r + k) % n, 7).Wait()
            rr.Wait()
            k <<= 1

    def Bcast(self, buf: torch.Tensor, root: int = 0, algo: Optional[str] = None):
        """``algo``: see "window collectives" below (None: the MPIT_COLLECTIVES variable)."""
        n = self.Get_size()
        if n == 1:
            return buf
        t = _flat(buf)
        algo = self._coll_algo(algo)
        if algo == "window":
            req = self._coll_bcast(t, root, keep=(buf,))
            if req is not None:
                req.Wait()
                return buf
        if algo != "p2p" and self._use_rccl(t):
            import torch.distributed as dist

            dist.broadcast(t, src=self._ranks[root], group=self._pg)
            return buf
        r = (self.Get_rank() - root) % n  # relative rank, binomial tree
        mask = 1
        while mask < n:
            if r & mask:
                self._crecv(t, (r - mask + root) % n, 1).Wait()
                break
            mask <<= 1
        mask >>= 1
        while mask > 0:
            if r + mask < n:
                self._csend(t, (r + mask + root) % n, 1).Wait()
            mask >>= 1
        return buf

    @_pair_call
    def Reduce(self, sendbuf, recvbuf, op: Op = SUM, root: int = 0, algo: Optional[str] = None, pairtype=None):
        """``algo``: see "window collectives" below (None: the MPIT_COLLECTIVES variable)."""
        n = self.Get_size()
        src = _flat(sendbuf)
        if n == 1:
            if recvbuf is not None and recvbuf is not sendbuf:
                _flat(recvbuf).copy_(src)
            return recvbuf
        algo = self._coll_algo(algo)
        if algo == "window":
            req = self._coll_reduce(src, recvbuf, op, root, keep=(sendbuf, recvbuf))
            if req is not None:
                req.Wait()
                return recvbuf
        if algo != "p2p" and self._use_rccl(src) and _rccl_op(op) is not None:
            import torch.distributed as dist

            acc = src.clone()
            dist.reduce(acc, dst=self._ranks[root], op=_rccl_op(op), group=self._pg)
            if self.Get_rank() == root:
                _flat(recvbuf).copy_(acc)
            return recvbuf
        me = self.Get_rank()
        if not op.commute:
            # ordered linear reduction at the root: ((b0 op b1) op b2) ...
            if me == root:
                parts = []
                for q in range(n):
                    if q == me:
                        parts.append(src.clone())
                    else:
                        tmp = torch.empty_like(src)
                        self._crecv(tmp, q, 2).Wait()
                        parts.append(tmp)
                acc = parts[0]
                for q in range(1, n):
                    acc = op(acc, parts[q])
                _flat(recvbuf).copy_(acc)
            else:
                self._csend(src, root, 2).Wait()
            return recvbuf
        acc = src.clone()
        tmp = torch.empty_like(src)
        r = (me - root) % n
        mask = 1
        while mask < n:
            if r & mask:
                self._csend(acc, (r - mask + root) % n, 2).Wait()
                break
            if r + mask < n:
                self._crecv(tmp, (r + mask + root) % n, 2).Wait()
                acc = op(acc, tmp)
            mask <<= 1
        if me == root:
            _flat(recvbuf).copy_(acc)
        return recvbuf

    @_pair_call
    def Allreduce(self, sendbuf, recvbuf=None, op: Op = SUM, algo: Optional[str] = None, pairtype=None):
        """MPI_Allreduce (mpifuncs.c:83). ``sendbuf is recvbuf`` (IN_PLACE) allowed.
        ``algo``: None (the MPIT_ALLREDUCE variable, default ``auto``) | ``auto`` (RCCL when
        every rank owns its GPU, else the point-to-point ring / tree) | ``p2p`` (the ring /
        tree always) | ``window`` (the peer-reduce kernel over symmetric memory, see
        :meth:`sym_alloc`; what it cannot run falls back to ``auto``)."""
        if recvbuf is None:
            recvbuf = sendbuf
        n = self.Get_size()
        src = _flat(sendbuf)
        dst = _flat(recvbuf)
        if n == 1:
            if dst.data_ptr() != src.data_ptr():
                dst.copy_(src)
            return recvbuf
        algo = self._ar_algo(algo)
        if algo == "window" and self._win_ok(src, dst, op):
            req = self._ar_submit(src, dst, op, keep=(sendbuf, recvbuf))
            if req is not None:
                req.Wait()
                return recvbuf
        if algo != "p2p" and self._use_rccl(src) and _rccl_op(op) is not None:
            import torch.distributed as dist

            if dst.data_ptr() != src.data_ptr():
                dst.copy_(src)
            dist.all_reduce(dst, op=_rccl_op(op), group=self._pg)
            self._ar_count("rccl")
            return recvbuf
        self._ar_count("p2p")
        if op.name in _ELEMENTWISE_OPS and n > 2 and src.numel() >= 64 * n:
            if dst.data_ptr() != src.data_ptr():
                dst.copy_(src)
            self._ring_allreduce(dst, op)
            return recvbuf
        tmp = torch.empty_like(src)
        self.Reduce(src, tmp, op, 0, algo="auto")
        if self.Get_rank() == 0:
            dst.copy_(tmp)
        self.Bcast(dst, 0, algo="auto")
        return recvbuf

    def _ring_allreduce(self, buf: torch.Tensor, op: Op):
        """Ring reduce-scatter + all-gather over the point-to-point layer (commutative
        ops): every rank sends and receives 2(n-1)/n of the buffer, with both of its
        neighbour links busy every step, instead of a binomial reduce + broadcast that
        moves the whole buffer log2(n) times through the root."""
        n, r = self.Get_size(), self.Get_rank()
        m = buf.numel()
        bounds = [m * k // n for k in range(n + 1)]
        chunk = [buf[bounds[k]: bounds[k + 1]] for k in range(n)]
        # two receive buffers: step s's op kernel (queued on the compute stream) may still
        # read tmp[s % 2] while step s + 1's receive lands — the engine pulls on its own
        # stream. Step s + 2 reuses it only after step s + 1's send synchronised the stream.
        cap = max(bounds[k + 1] - bounds[k] for k in range(n))
        tmps = [torch.empty(cap, dtype=buf.dtype, device=buf.device) for _ in range(2)]
        right, left = (r + 1) % n, (r - 1) % n
        for s in range(n - 1):  # reduce-scatter: rank r ends owning chunk (r + 1) % n
            si, ri = (r - s) % n, (r - s - 1) % n
            t = tmps[s % 2][: chunk[ri].numel()]
            rq = self._crecv(t, left, 10)
            sq = self._csend(chunk[si], right, 10)
            rq.Wait()
            chunk[ri].copy_(op(chunk[ri], t))
            sq.Wait()
        for s in range(n - 1):  # all-gather of the reduced chunks
            si, ri = (r + 1 - s) % n, (r - s) % n
            rq = self._crecv(chunk[ri], left, 11)
            sq = self._csend(chunk[si], right, 11)
            rq.Wait()
            sq.Wait()

    @_pair_call
    def Iallreduce(self, sendbuf, recvbuf=None, op: Op = SUM, algo: Optional[str] = None, pairtype=None) -> Request:
        """Non-blocking all-reduce (mpifuncs.c:1357). RCCL work handle on HBM tensors,
        a background progress thread otherwise; ``algo="window"``: a ticket in the
        communicator's all-reduce FIFO (:meth:`Allreduce`, :meth:`_ar_submit`)."""
        if recvbuf is None:
            recvbuf = sendbuf
        src = _flat(sendbuf)
        algo = self._ar_algo(algo)
        if self.Get_size() > 1 and algo == "window" and self._win_ok(src, _flat(recvbuf), op):
            req = self._ar_submit(src, _flat(recvbuf), op, keep=(sendbuf, recvbuf))
            if req is not None:
                return req
        if self.Get_size() == 1:
            # one rank: the reduction is the rank's own data — a stream-ordered copy (or
            # nothing, in place), complete at once; no background thread per call
            dst = _flat(recvbuf)
            if dst.data_ptr() != src.data_ptr():
                dst.copy_(src)
            return Request(self, keep=(sendbuf, recvbuf))
        if algo != "p2p" and self._use_rccl(src) and _rccl_op(op) is not None:
            import torch.distributed as dist

            dst = _flat(recvbuf)
            if dst.data_ptr() != src.data_ptr():
                dst.copy_(src)
            w = dist.all_reduce(dst, op=_rccl_op(op), group=self._pg, async_op=True)
            self._ar_count("rccl")
            return Request(self, work=w, keep=(sendbuf, recvbuf))
        fb = "p2p" if algo == "p2p" else "auto"  # (a window request that cannot run is today's routing)
        return self._bg(lambda: self.Allreduce(sendbuf, recvbuf, op, algo=fb), keep=(sendbuf, recvbuf))

    # ---------------------------------------------------------------- window all-reduce
    # Symmetric memory + the peer-reduce kernel (csrc/kernels/allreduce.hip) + the two-barrier
    # protocol of csrc/core/window.cpp Window::allreduce. Every call of this section is
    # collective over the communicator and must be made in the same order, with the same
    # registration state of its buffers, on every member.
    def _ar_algo(self, algo: Optional[str]) -> str:
        a = (algo if algo is not None else os.environ.get("MPIT_ALLREDUCE", "")) or "auto"
        if a not in ("auto", "window", "p2p"):
            raise ValueError(f"all-reduce algo must be auto, window or p2p, not {a!r}")
        return a

    def _ar_count(self, path: str):
        with self._ar_lock:
            self._ar_calls[path] += 1

    def ar_stats(self) -> dict:
        """All-reduce calls of this communicator per path: ``window`` (of which
        ``window_staged`` went through the staging buffer), ``p2p``, ``rccl``."""
        with self._ar_lock:
            return dict(self._ar_calls)

    def sym_alloc(self, numel: int, dtype=torch.float32, device=None) -> torch.Tensor:
        """Collective: a tensor of ``numel`` elements backed by a window every member maps (HBM
        through HIP IPC, or host shm with ``device=False`` / on ranks without a GPU). All-reduces
        with ``algo="window"`` on it, or on any contiguous view inside it, run in place."""
        from .window import Win

        if device is None:
            dev = _rt.device() is not None
        elif isinstance(device, bool):
            dev = device
        else:
            dev = torch.device(device).type == "cuda"
        win = Win.Allocate(int(numel), dtype, comm=self, device=dev)
        return self._sym_add(win, win.tensor, True)

    def sym_register(self, tensor: torch.Tensor) -> torch.Tensor:
        """Collective: expose an existing HBM tensor zero-copy (``Win.Create``)."""
        from .window import Win

        if not tensor.is_cuda:
            raise ValueError("sym_register exposes HBM tensors in place; host memory comes from sym_alloc")
        return self._sym_add(Win.Create(tensor, self), tensor, False)

    def _sym_add(self, win, t: torch.Tensor, owned: bool) -> torch.Tensor:
        # Window::allreduce reports "unsupported" per rank (a member it could not map); agree on it
        # here, collectively, so that every member falls back together instead of one of them
        # failing while its peers wait in the protocol's barrier
        if not all(self.allgather_obj(bool(win._w.allreduce_capable))):
            self._ar_off = True
        self._sym.append(_SymRec(t.data_ptr(), t.data_ptr() + _nbytes(t), win, t, owned))
        return t

    def _sym_find(self, t: torch.Tensor):
        """(record, byte offset) of the registered range that holds all of ``t``, or None."""
        p, nb = t.data_ptr(), _nbytes(t)
        for rec in self._sym:
            if rec.lo <= p and p + nb <= rec.hi and rec.tensor.device == t.device:
                return rec, p - rec.lo
        return None

    def sym_free(self, tensor: Optional[torch.Tensor] = None):
        """Collective: release the symmetric range that holds ``tensor`` (all of them: None)."""
        if tensor is None:
            recs = list(self._sym)
        else:
            hit = self._sym_find(tensor)
            if hit is None:
                raise ValueError("sym_free: not a symmetric tensor of this communicator")
            recs = [hit[0]]
        self._ar_drain()
        self.Barrier()  # no member is still inside an all-reduce on it
        for rec in recs:
            self._sym.remove(rec)
            for k, st in list(self._ar_stage.items()):
                if st.data_ptr() == rec.lo:
                    del self._ar_stage[k]
            rec.win.Free()

    def _win_ok(self, src: torch.Tensor, dst: torch.Tensor, op: Op) -> bool:
        code, dt = _pr_codes(op, src.dtype)
        if code is None or dt is None or self.Get_size() > 8 or self._rank == UNDEFINED or self._ar_off:
            return False
        if dst.dtype != src.dtype or dst.device != src.device or dst.numel() != src.numel():
            return False
        if src.is_cuda and src.device != _rt.device():
            return False
        return bool(native().peer_reduce_supported(code, dt))

    @staticmethod
    def _ar_stage_bytes() -> int:
        return max(4096, int(float(os.environ.get("MPIT_AR_STAGE_MB", "32")) * (1 << 20))) & ~15

    def _ar_staging(self, kind: str) -> torch.Tensor:
        st = self._ar_stage.get(kind)
        if st is None:
            st = self._ar_stage[kind] = self.sym_alloc(self._ar_stage_bytes(), torch.uint8, device=(kind == "cuda"))
        return st

    def _ar_submit(self, src: torch.Tensor, dst: torch.Tensor, op: Op, keep=()) -> Request:
        """Take a ticket in the communicator's all-reduce FIFO (on the caller's thread, so the
        order is the call order on every rank). The ticket carries an event recorded on the
        caller's current stream; the worker makes the communicator's own stream wait for it and
        runs the blocking protocol there. Completion means complete for every stream.
        None (on every member alike): the window path is off for this communicator, the caller
        falls back to today's routing."""
        kind = "cuda" if src.is_cuda else "cpu"
        inplace = src.data_ptr() == dst.data_ptr()
        hit = self._sym_find(src)
        disjoint = inplace or src.data_ptr() + _nbytes(src) <= dst.data_ptr() or \
            dst.data_ptr() + _nbytes(dst) <= src.data_ptr()
        if hit is not None and inplace:
            plan = ("direct", hit[0].win, hit[1])
        elif hit is not None and disjoint and self._sym_find(dst) is None and \
                _nbytes(src) <= native().ar_oneshot_bytes():
            plan = ("oneshot", hit[0].win, hit[1])  # straight into the caller's destination
        else:
            st = self._ar_staging(kind)  # (created collectively, here on the caller's thread)
            if self._ar_off:  # (agreed while creating it: a member cannot map the staging window)
                return None
            plan = ("staged", self._sym_find(st)[0].win, st)
        ev = None
        if kind == "cuda":
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(src.device))
        req = Request(self, keep=keep, event=threading.Event())
        self._ar_start()
        self._ar_count("window")
        if plan[0] == "staged":
            self._ar_count("window_staged")
        self._ar_q.put((plan, src, dst) + _pr_codes(op, src.dtype) + (ev, req))
        return req

    def _ar_start(self):
        """The FIFO worker of the window all-reduce and the window collectives (one per communicator)."""
        import queue

        if self._ar_thread is None:
            self._ar_q = queue.Queue()
            if _rt.device() is not None:
                self._ar_stream = torch.cuda.Stream(_rt.device())
            self._ar_thread = threading.Thread(target=self._ar_worker, args=(self._ar_q,), daemon=True,
                                               name=f"mpit-allreduce-{self._ctx}")
            self._ar_thread.start()

    def _ar_worker(self, q):
        if _rt.device() is not None:
            torch.cuda.set_device(_rt.device())
        while True:
            item = q.get()
            if item is None:
                q.task_done()
                return
            req = item[-1]
            try:
                if item[0] == "coll":
                    self._coll_exec(item[1], item[2])
                else:
                    self._ar_exec(*item[:-1])
            except BaseException as e:  # surfaced by Wait / Test
                req._err = e
            req._ev.set()
            q.task_done()

    def _ar_exec(self, plan, src, dst, code, dt, ev):
        n, es = src.numel(), src.element_size()
        if ev is None:
            self._ar_run(plan, src, dst, code, dt, n, es, 0, None)
            return
        s = self._ar_stream
        with torch.cuda.stream(s):
            ev.wait(s)  # what the caller queued before the call, and nothing later
            self._ar_run(plan, src, dst, code, dt, n, es, s.cuda_stream, s)

    def _ar_run(self, plan, src, dst, code, dt, n, es, sptr, stream):
        how, win = plan[0], plan[1]._w
        if how == "direct":
            ok = win.allreduce(plan[2], n, dt, code, sptr, 0, 0)
        elif how == "oneshot":
            ok = win.allreduce(plan[2], n, dt, code, sptr, 1, dst.data_ptr())
        else:
            stage = plan[2]
            cap = stage.numel() // es
            ok, i = True, 0
            while ok and i < n:
                m = min(cap, n - i)
                sv = stage[: m * es].view(src.dtype)
                sv.copy_(src[i: i + m])
                ok = win.allreduce(0, m, dt, code, sptr, 0, 0)
                dst[i: i + m].copy_(sv)
                i += m
            if stream is not None:
                stream.synchronize()
        if not ok:
            # (not reachable through sym_alloc / sym_register: they agree on the capability and
            # switch the communicator to the fallback before any ticket is taken)
            raise RuntimeError("mpit: this window cannot run the peer-reduce all-reduce (member not mapped)")

    def _ar_drain(self):
        if self._ar_q is not None:
            self._ar_q.join()

    def _ar_stop(self):
        if self._ar_thread is not None:
            self._ar_q.put(None)
            self._ar_thread.join()
            self._ar_thread = self._ar_q = None

    # ---------------------------------------------------------------- window collectives
    # Reduce_scatter(_block), Allgather(v), Alltoall, Bcast, Reduce, Scan, Exscan and the I* forms
    # of the first five take ``algo``: ``auto`` (the routing without this section: RCCL when every
    # rank owns its GPU, else the point-to-point algorithms), ``p2p`` (the point-to-point
    # algorithms always) or ``window``; None reads the MPIT_COLLECTIVES variable (default
    # ``auto``; MPIT_ALLREDUCE stays the all-reduce's alone). ``window``: one kernel launch
    # (csrc/kernels/peer_coll.hip) between the two barriers of csrc/core/window.cpp
    # Window::pull_gather / pull_fold / scan over symmetric memory, bitwise reproducible (member
    # order is fold order). Every such call takes a ticket in the FIFO of the window all-reduce
    # (:meth:`_ar_submit`): the same worker, the same stream, an event recorded on the caller's
    # stream, so all-reduces and these collectives stay in call order on every rank and share the
    # one staging window safely. Eligibility is the same on every rank: 2..8 members, a supported
    # (op, dtype) for the folding ones, no member unable to map a window (``_ar_off``), tensors
    # on this rank's device or on the host; what is not eligible takes ``auto`` on every member
    # alike (counted as ``fallback`` in :meth:`coll_stats`).
    # The contract is Allreduce's: the same call order, and the same registration state and
    # in-place-ness of the buffers on every member (a buffer inside a symmetric range lies at the
    # same offset of that range everywhere). A buffer inside a symmetric range (:meth:`sym_alloc`,
    # :meth:`sym_register`) is read in place by the other members; anything else goes through the
    # staging window (MPIT_AR_STAGE_MB) in pieces, and ``sendbuf`` is never modified. A rank whose
    # part is empty still passes a (zero-length) view of its symmetric buffer, so that it takes
    # the same plan as its peers.
    def _coll_algo(self, algo: Optional[str]) -> str:
        a = (algo if algo is not None else os.environ.get("MPIT_COLLECTIVES", "")) or "auto"
        if a not in ("auto", "window", "p2p"):
            raise ValueError(f"collective algo must be auto, window or p2p, not {a!r}")
        return a

    def coll_stats(self) -> dict:
        """Calls with ``algo="window"`` per collective: ``window`` (of which ``window_staged`` went
        through the staging buffer) and ``fallback`` (not eligible: today's routing)."""
        with self._ar_lock:
            return {k: dict(v) for k, v in self._coll_calls.items()}

    def _coll_count(self, name: str, path: str):
        with self._ar_lock:
            (self._coll_calls if name in self._coll_calls else self._vcoll_calls)[name][path] += 1

    @staticmethod
    def _addr(t: torch.Tensor) -> int:
        """The byte address of ``t``'s first element, of an empty view too (whose data_ptr() is 0)."""
        return t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size()

    def _coll_sym(self, t: torch.Tensor, numel: Optional[int] = None):
        """(native window, byte offset) of the symmetric range holding the first ``numel``
        elements of ``t``, or None."""
        p = self._addr(t)
        nb = (t.numel() if numel is None else numel) * t.element_size()
        for rec in self._sym:
            if rec.lo <= p and p + nb <= rec.hi and rec.tensor.device == t.device:
                return rec.win._w, p - rec.lo
        return None

    def _coll_ok(self, name: str, tensors, op: Optional[Op] = None) -> bool:
        ok = 2 <= self.Get_size() <= 8 and self._rank != UNDEFINED and not self._ar_off
        t0 = tensors[0]
        for t in tensors:
            ok = ok and t.dtype == t0.dtype and t.device == t0.device
        ok = ok and (not t0.is_cuda or t0.device == _rt.device())
        if ok and op is not None:
            code, dt = _pr_codes(op, t0.dtype)
            ok = code is not None and dt is not None and bool(native().peer_reduce_supported(code, dt))
        if not ok:
            self._coll_count(name, "fallback")
        return ok

    def _coll_overlap(self, a: torch.Tensor, na: int, b: torch.Tensor, nb: int) -> bool:
        pa, pb = self._addr(a), self._addr(b)
        return na > 0 and nb > 0 and pa < pb + nb * b.element_size() and pb < pa + na * a.element_size()

    def _coll_stage(self, name: str, like: torch.Tensor):
        """(native staging window, staging tensor), created collectively on the caller's thread;
        None (on every member alike) when a member cannot map it."""
        st = self._ar_staging("cuda" if like.is_cuda else "cpu")
        if self._ar_off:
            self._coll_count(name, "fallback")
            return None
        return self._sym_find(st)[0].win._w, st

    def _coll_submit(self, name: str, staged: bool, fn, like: torch.Tensor, keep=()) -> Request:
        """A ticket in the all-reduce FIFO for ``fn(stream pointer, torch stream or None)``."""
        ev = None
        if like.is_cuda:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(like.device))
        req = Request(self, keep=keep, event=threading.Event())
        self._ar_start()
        self._coll_count(name, "window")
        if staged:
            self._coll_count(name, "window_staged")
        self._ar_q.put(("coll", fn, ev, req))
        return req

    def _coll_exec(self, fn, ev):
        if ev is None:
            fn(0, None)
            return
        s = self._ar_stream
        with torch.cuda.stream(s):
            ev.wait(s)  # what the caller queued before the call, and nothing later
            fn(s.cuda_stream, s)
            s.synchronize()

    @staticmethod
    def _coll_done(ok: bool):
        if not ok:  # (not reachable: the capability is agreed on before any ticket is taken)
            raise RuntimeError("mpit: this window cannot run the window collectives (member not mapped)")

    def _coll_reduce_scatter(self, src, dst, counts, op, keep=()) -> Optional[Request]:
        n, me = self.Get_size(), self.Get_rank()
        if counts is None:
            counts = [src.numel() // n] * n
        if not self._coll_ok("reduce_scatter", (src, dst), op):
            return None
        counts = [int(c) for c in counts]
        total, mine, d0 = sum(counts), counts[me], sum(counts[:me])
        if src.numel() < total or dst.numel() < mine:
            raise ValueError("Reduce_scatter: buffer shorter than its counts")
        if self._coll_overlap(src, total, dst, mine):
            raise ValueError("Reduce_scatter(algo='window'): recvbuf overlaps sendbuf")
        es, (code, dt) = src.element_size(), _pr_codes(op, src.dtype)
        out = self._addr(dst)
        hit = self._coll_sym(src, total)
        if hit is not None:
            win, off = hit

            def fn(sptr, stream):
                self._coll_done(win.pull_fold(off + d0 * es, mine, dt, code, out if mine else 0, 0, n, sptr))
        else:
            plan = self._coll_stage("reduce_scatter", src)
            if plan is None:
                return None
            win, st = plan
            cap = st.numel() // es

            def fn(sptr, stream):
                for i in range(0, total, cap):
                    m = min(cap, total - i)
                    st[: m * es].view(src.dtype).copy_(src[i: i + m])
                    lo, hi = max(i, d0), min(i + m, d0 + mine)
                    if hi > lo:
                        ok = win.pull_fold((lo - i) * es, hi - lo, dt, code, out + (lo - d0) * es, 0, n, sptr)
                    else:
                        ok = win.pull_fold(0, 0, dt, code, 0, 0, n, sptr)
                    self._coll_done(ok)
        return self._coll_submit("reduce_scatter", hit is None, fn, src, keep)

    def _coll_reduce(self, src, recvbuf, op, root, keep=()) -> Optional[Request]:
        n, me = self.Get_size(), self.Get_rank()
        dst = _flat(recvbuf) if me == root else None
        if not self._coll_ok("reduce", (src,) if dst is None else (src, dst), op):
            return None
        total = src.numel()
        if dst is not None and dst.numel() < total:
            raise ValueError("Reduce: recvbuf shorter than sendbuf")
        if dst is not None and self._coll_overlap(src, total, dst, total):
            raise ValueError("Reduce(algo='window'): recvbuf overlaps sendbuf")
        es, (code, dt) = src.element_size(), _pr_codes(op, src.dtype)
        out = self._addr(dst) if dst is not None else 0
        hit = self._coll_sym(src)
        if hit is not None:
            win, off = hit

            def fn(sptr, stream):
                self._coll_done(win.pull_fold(off, total, dt, code, out, 0, n, sptr))
        else:
            plan = self._coll_stage("reduce", src)
            if plan is None:
                return None
            win, st = plan
            cap = st.numel() // es

            def fn(sptr, stream):
                for i in range(0, total, cap):
                    m = min(cap, total - i)
                    st[: m * es].view(src.dtype).copy_(src[i: i + m])
                    self._coll_done(win.pull_fold(0, m, dt, code, out + i * es if out else 0, 0, n, sptr))
        return self._coll_submit("reduce", hit is None, fn, src, keep)

    def _coll_allgather(self, src, dst, counts, displs, keep=()) -> Optional[Request]:
        n, me = self.Get_size(), self.Get_rank()
        if not self._coll_ok("allgather", (src, dst)):
            return None
        if counts is None:
            counts = [src.numel()] * n
        counts = [int(c) for c in counts]
        if displs is None:
            displs = [sum(counts[:i]) for i in range(n)]
        extent = max(d + c for d, c in zip(displs, counts))
        if dst.numel() < extent or src.numel() < counts[me]:
            raise ValueError("Allgatherv: buffer shorter than its counts")
        es = src.element_size()
        out = self._addr(dst)
        hitd = self._coll_sym(dst, extent)
        hit, staged = None, False
        if hitd is not None and self._addr(src) == out + displs[me] * es:
            # in place: my segment of the symmetric recvbuf is my contribution; pull the others'
            win, off = hitd
            segs = [(g, off + displs[g] * es, out + displs[g] * es, counts[g] * es) for g in range(n) if g != me]
        else:
            if self._coll_overlap(src, counts[me], dst, extent):
                raise ValueError("Allgatherv(algo='window'): sendbuf overlaps recvbuf and is not this rank's segment")
            hit = self._coll_sym(src, counts[me])
            if hit is not None:
                win, off = hit
                segs = [(g, off, out + displs[g] * es, counts[g] * es) for g in range(n)]
            else:
                staged = True
        if not staged:
            def fn(sptr, stream):
                self._coll_done(win.pull_gather(segs, sptr))
        else:
            plan = self._coll_stage("allgather", src)
            if plan is None:
                return None
            win, st = plan
            cap = st.numel() // es

            def fn(sptr, stream):
                for i in range(0, max(counts), cap):
                    if counts[me] > i:
                        m = min(cap, counts[me] - i)
                        st[: m * es].view(src.dtype).copy_(src[i: i + m])
                    sg = [(g, 0, out + (displs[g] + i) * es, min(cap, counts[g] - i) * es)
                          for g in range(n) if counts[g] > i]
                    self._coll_done(win.pull_gather(sg, sptr))
        return self._coll_submit("allgather", staged, fn, src, keep)

    def _coll_alltoall(self, src, dst, keep=()) -> Optional[Request]:
        n, me = self.Get_size(), self.Get_rank()
        if not self._coll_ok("alltoall", (src, dst)):
            return None
        c = src.numel() // n
        if dst.numel() < c * n:
            raise ValueError("Alltoall: recvbuf shorter than sendbuf")
        if self._coll_overlap(src, c * n, dst, c * n):
            raise ValueError("Alltoall(algo='window'): recvbuf overlaps sendbuf")
        es = src.element_size()
        out = self._addr(dst)
        hit = self._coll_sym(src, c * n)
        if hit is not None:
            win, off = hit
            segs = [(g, off + me * c * es, out + g * c * es, c * es) for g in range(n)]

            def fn(sptr, stream):
                self._coll_done(win.pull_gather(segs, sptr))
        else:
            plan = self._coll_stage("alltoall", src)
            if plan is None:
                return None
            win, st = plan
            cap = st.numel() // es

            def fn(sptr, stream):
                for i in range(0, c * n, cap):  # pieces of the flat send buffer; block `me` of each is mine
                    m = min(cap, c * n - i)
                    st[: m * es].view(src.dtype).copy_(src[i: i + m])
                    lo, hi = max(i, me * c), min(i + m, (me + 1) * c)
                    sg = [(g, (lo - i) * es, out + (g * c + lo - me * c) * es, (hi - lo) * es)
                          for g in range(n)] if hi > lo else []
                    self._coll_done(win.pull_gather(sg, sptr))
        return self._coll_submit("alltoall", hit is None, fn, src, keep)

    def _coll_bcast(self, t, root, keep=()) -> Optional[Request]:
        me = self.Get_rank()
        if not self._coll_ok("bcast", (t,)):
            return None
        es, total = t.element_size(), t.numel()
        out = self._addr(t)
        hit = self._coll_sym(t)
        if hit is not None:
            win, off = hit
            segs = [(root, off, out, total * es)] if me != root else []

            def fn(sptr, stream):
                self._coll_done(win.pull_gather(segs, sptr))
        else:
            plan = self._coll_stage("bcast", t)
            if plan is None:
                return None
            win, st = plan
            cap = st.numel() // es

            def fn(sptr, stream):
                for i in range(0, total, cap):  # the root stages a piece, the others pull it into place
                    m = min(cap, total - i)
                    if me == root:
                        st[: m * es].view(t.dtype).copy_(t[i: i + m])
                    sg = [(root, 0, out + i * es, m * es)] if me != root else []
                    self._coll_done(win.pull_gather(sg, sptr))
        return self._coll_submit("bcast", hit is None, fn, t, keep)

    def _coll_scan(self, src, dst, op, excl: bool, keep=()) -> Optional[Request]:
        me = self.Get_rank()
        name = "exscan" if excl else "scan"
        if not self._coll_ok(name, (src, dst), op):
            return None
        total = src.numel()
        if dst.numel() < total:
            raise ValueError("Scan: recvbuf shorter than sendbuf")
        inplace = self._addr(src) == self._addr(dst)
        if not inplace and self._coll_overlap(src, total, dst, total):
            raise ValueError("Scan(algo='window'): recvbuf overlaps sendbuf")
        es, (code, dt) = src.element_size(), _pr_codes(op, src.dtype)
        hit = self._coll_sym(src) if inplace else None
        if hit is not None:
            win, off = hit

            def fn(sptr, stream):
                self._coll_done(win.scan(off, total, dt, code, excl, sptr))
        else:
            plan = self._coll_stage(name, src)
            if plan is None:
                return None
            win, st = plan
            cap = st.numel() // es

            def fn(sptr, stream):
                for i in range(0, total, cap):
                    m = min(cap, total - i)
                    sv = st[: m * es].view(src.dtype)
                    sv.copy_(src[i: i + m])
                    self._coll_done(win.scan(0, m, dt, code, excl, sptr))
                    if not (excl and me == 0):  # rank 0 of Exscan: recvbuf untouched, as MPI says
                        dst[i: i + m].copy_(sv)
        return self._coll_submit(name, hit is None, fn, src, keep)

    # ---------------------------------------------------------------- irregular window collectives
    # Gatherv / Gather, Scatterv / Scatter, Alltoallv and Alltoallw with ``algo="window"``: a rank
    # cannot know a peer's displacements, counts or tensor layouts, so every member first publishes
    # them: one fixed-size int64 record per member (a header and, per peer, where the segment sent
    # to it lies: the symmetric range and byte offset, the bytes, the loops and run length of
    # :func:`datatypes.layout_of`, plus the bytes expected from that peer), exchanged in ONE host
    # Allgather (``algo="auto"``) on the caller's thread before any ticket. Every decision and
    # every refusal is taken from the exchanged records alone, so all members take the same path
    # or raise the same ValueError, and nobody is left waiting in the protocol's barrier.
    # Paths: *in place* when every non-empty send segment lies in one symmetric range (peers read
    # it where it lies: Window::pull_gather when every segment of the call is contiguous,
    # Window::pull_plan, one peer_plan_gather launch, csrc/kernels/peer_plan.hip, as soon as one is
    # strided; a rank's own part is a local segment of the same launch); *staged* when not and
    # every member's send stream (each segment padded to 16 bytes) fits the staging window
    # (MPIT_AR_STAGE_MB), packed there in one piece by type_copy; else the *fallback*, today's
    # routing, on every member alike. Gatherv: the root alone pulls; Scatterv: every rank pulls its
    # piece from the root. ``sendbuf`` is never modified. Counted in :meth:`vcoll_stats`.
    _VREC = 12  # int64 per send record: range, offset, bytes, loop count, 3 x (n, stride), run length, spare

    def vcoll_stats(self) -> dict:
        """Calls with ``algo="window"`` of Gatherv / Gather (``gatherv``), Scatterv / Scatter
        (``scatterv``), ``alltoallv`` and ``alltoallw``: ``window`` (of which ``window_staged`` went
        through the staging buffer) and ``fallback`` (not eligible: today's routing)."""
        with self._ar_lock:
            return {k: dict(v) for k, v in self._vcoll_calls.items()}

    def _vcoll_span(self, buf: torch.Tensor, displ, count):
        """buf[displ: displ + count], or None when that lies outside buf (a slice would clamp)."""
        displ, count = int(displ), int(count)
        if displ < 0 or count < 0 or displ + count > buf.numel():
            return None
        return buf[displ: displ + count]

    def _vcoll(self, name: str, sends, recvs, err: int, keep=()) -> Optional[Request]:
        """``sends[q]`` / ``recvs[q]``: the tensor (any strides) this rank sends to / receives from
        member q, or None for nothing; ``err``: a _VCOLL_ERRORS code the caller found. A Request, or
        None on every member alike (the fallback)."""
        from .datatypes import layout_of, run_plan, _bytes_at

        n, me, V = self.Get_size(), self.Get_rank(), self._VREC
        if not (2 <= n <= 8 and self._rank != UNDEFINED and not self._ar_off):
            self._coll_count(name, "fallback")
            return None
        tensors = [t for t in list(sends) + list(recvs) if t is not None]
        ok = all(t.device == tensors[0].device for t in tensors)
        ok = ok and all(not t.is_cuda or t.device == _rt.device() for t in tensors)
        kind = 0 if not tensors else (2 if tensors[0].is_cuda else 1)
        # ---- my record
        rec = torch.zeros(4 + (V + 1) * n, dtype=torch.int64)
        splans, rplans, spans = [None] * n, [None] * n, []
        for q in range(n):
            for side, t in ((0, sends[q]), (1, recvs[q])):
                if t is None or t.numel() == 0:
                    continue
                try:
                    plan = layout_of(t)
                except ValueError:
                    err = err or 2
                    continue
                addr = self._addr(t)
                spans.append((side, q, addr, addr + plan.hi, plan.loops, plan.L))
                if side == 1:
                    if plan.self_overlap():
                        err = err or 4
                    rplans[q] = (addr, plan)
                    rec[4 + V * n + q] = plan.total
                    rec[3] |= int(bool(plan.loops))
                    continue
                splans[q] = plan
                sym = -1
                for k, sr in enumerate(self._sym):
                    if sr.lo <= addr and addr + plan.hi <= sr.hi and sr.tensor.device == t.device:
                        sym, addr = k, addr - sr.lo
                        break
                loops = [x for ns in plan.loops for x in ns] + [0] * (6 - 2 * len(plan.loops))
                rec[4 + V * q: 4 + V * (q + 1)] = torch.tensor([sym, addr if sym >= 0 else 0, plan.total, len(plan.loops)]
                                                              + loops + [plan.L, 0])
        for _, qd, dlo, dhi, dloops, dl in (x for x in spans if x[0] == 1):
            for _, qs, slo, shi, sloops, sl in (x for x in spans if x[0] == 0):
                own = qd == me and qs == me and dlo == slo and dloops == sloops and dl == sl
                if dlo < shi and slo < dhi and not own:
                    err = err or 3
        rec[0], rec[1], rec[2] = err, int(ok), kind
        # ---- the exchange, and what every member reads from it alike
        every = torch.zeros(n * rec.numel(), dtype=torch.int64)
        self.Allgather(rec, every, algo="auto")
        every = every.view(n, -1).tolist()
        kinds = {m[2] for m in every if m[2]}
        if not all(m[1] for m in every) or len(kinds) > 1:
            self._coll_count(name, "fallback")
            return None
        for s, m in enumerate(every):
            if m[0]:
                raise ValueError(f"{name}(algo='window'): rank {s}: {_VCOLL_ERRORS.get(m[0], m[0])}")
        S = [[m[4 + V * q: 4 + V * (q + 1)] for q in range(n)] for m in every]  # S[s][q]: s sends to q
        for s in range(n):
            for q in range(n):
                if S[s][q][2] != every[q][4 + V * n + s]:
                    raise ValueError(f"{name}(algo='window'): rank {s} sends {S[s][q][2]} bytes to rank {q}, "
                                     f"which expects {every[q][4 + V * n + s]}")
        cuda = kinds == {2}
        like = tensors[0] if tensors else torch.empty(0, device=_rt.device() if cuda else "cpu")
        live = [S[s][q] for s in range(n) for q in range(n) if S[s][q][2]]
        ranges = {r[0] for r in live}
        strided_recv = any(m[3] for m in every)
        staged = not live or len(ranges) != 1 or -1 in ranges
        if staged:
            # member s's stream: its segments in peer order, each padded to 16 bytes
            soff = [[sum((S[s][p][2] + 15) & ~15 for p in range(q)) for q in range(n + 1)] for s in range(n)]
            if max(o[n] for o in soff) > self._ar_stage_bytes():
                self._coll_count(name, "fallback")
                return None
            stage = self._coll_stage(name, like)
            if stage is None:
                return None
            win, st = stage
            use_plan = strided_recv
        else:
            win, st = self._sym[ranges.pop()].win._w, None
            use_plan = strided_recv or any(r[3] for r in live)
        # ---- what this rank pulls: from member s, the segment it sends to me
        segs = []
        for s in range(n):
            r = S[s][me]
            if not r[2]:
                continue
            dst, dplan = rplans[s]
            if staged:
                off, sloops, sl = soff[s][me], [], r[2]
            else:
                off, sloops, sl = r[1], [[r[4 + 2 * k], r[5 + 2 * k]] for k in range(r[3])], r[10]
            if use_plan:
                shi = sl + sum((a - 1) * b for a, b in sloops)
                segs.append((s, off, (sloops, 0, 1, sl, sl, 16, 0, shi), dst,
                             ([list(x) for x in dplan.loops], 0, 1, dplan.L, dplan.L, 16, 0, dplan.hi)))
            else:
                segs.append((s, off, dst, r[2]))

        def fn(sptr, stream):
            if staged:
                for q in range(n):
                    if splans[q] is not None:  # pack (or copy) my segment for q into my stream
                        run_plan(splans[q], 0, _bytes_at(sends[q]), st[soff[me][q]: soff[me][q] + splans[q].total])
            self._coll_done(win.pull_plan(segs, sptr) if use_plan else win.pull_gather(segs, sptr))
        return self._coll_submit(name, staged, fn, like, keep)

    def _vcoll_gatherv(self, src, recvbuf, counts, displs, root, keep=()) -> Optional[Request]:
        n, me = self.Get_size(), self.Get_rank()
        sends, recvs, err = [None] * n, [None] * n, 0
        if me != root:
            sends[root] = src
        else:
            dst = _flat(recvbuf)
            if counts is None:
                counts = [src.numel()] * n
            if displs is None:
                displs = [sum(counts[:i]) for i in range(n)]
            for q in range(n):
                recvs[q] = self._vcoll_span(dst, displs[q], counts[q])
                err = err or int(recvs[q] is None)
            sends[me] = self._vcoll_span(src, 0, counts[me])
            err = err or int(sends[me] is None)
        return self._vcoll("gatherv", sends, recvs, err, keep)

    def _vcoll_scatterv(self, sendbuf, dst, counts, displs, root, keep=()) -> Optional[Request]:
        n, me = self.Get_size(), self.Get_rank()
        sends, recvs, err = [None] * n, [None] * n, 0
        if me != root:
            recvs[root] = dst
        else:
            src = _flat(sendbuf)
            if counts is None:
                counts = [dst.numel()] * n
            if displs is None:
                displs = [sum(counts[:i]) for i in range(n)]
            for q in range(n):
                sends[q] = self._vcoll_span(src, displs[q], counts[q])
                err = err or int(sends[q] is None)
            recvs[me] = self._vcoll_span(dst, 0, counts[me])
            err = err or int(recvs[me] is None)
        return self._vcoll("scatterv", sends, recvs, err, keep)

    def _vcoll_alltoallv(self, src, sendcounts, sdispls, dst, recvcounts, rdispls, keep=()) -> Optional[Request]:
        n = self.Get_size()
        sends = [self._vcoll_span(src, sdispls[q], sendcounts[q]) for q in range(n)]
        recvs = [self._vcoll_span(dst, rdispls[q], recvcounts[q]) for q in range(n)]
        err = int(any(t is None for t in sends + recvs))
        return self._vcoll("alltoallv", sends, recvs, err, keep)

    def _bg(self, fn, keep=()) -> Request:
        req = Request(self, keep=keep)
        with _coll_cv:
            ticket = _coll_tickets[0]
            _coll_tickets[0] += 1

        def run():
            with _coll_cv:
                _coll_cv.wait_for(lambda: _coll_tickets[1] == ticket)
            try:
                fn()
            except BaseException as e:  # surfaced by Wait/Test
                req._err = e
            finally:
                with _coll_cv:
                    _coll_tickets[1] += 1
                    _coll_cv.notify_all()

        th = threading.Thread(target=run, daemon=True)
        req._thread = th
        th.start()
        return req

    def Ibarrier(self) -> Request:
        return self._bg(self.Barrier)

    # The non-blocking forms of the collectives with a window path: with ``algo="window"`` the
    # ticket's Request (the FIFO of the window all-reduce, no thread per call); otherwise, and for
    # what the window path cannot run, the blocking call on a background thread as before.
    def Ibcast(self, buf, root=0, algo: Optional[str] = None) -> Request:
        algo = self._coll_algo(algo)
        if algo == "window" and self.Get_size() > 1:
            req = self._coll_bcast(_flat(buf), root, keep=(buf,))
            if req is not None:
                return req
        fb = "p2p" if algo == "p2p" else "auto"
        return self._bg(lambda: self.Bcast(buf, root, algo=fb), keep=(buf,))

    @_pair_call
    def Ireduce(self, sendbuf, recvbuf, op=SUM, root=0, algo: Optional[str] = None, pairtype=None) -> Request:
        algo = self._coll_algo(algo)
        if algo == "window" and self.Get_size() > 1:
            req = self._coll_reduce(_flat(sendbuf), recvbuf, op, root, keep=(sendbuf, recvbuf))
            if req is not None:
                return req
        fb = "p2p" if algo == "p2p" else "auto"
        return self._bg(lambda: self.Reduce(sendbuf, recvbuf, op, root, algo=fb), keep=(sendbuf, recvbuf))

    def Iallgather(self, sendbuf, recvbuf, algo: Optional[str] = None) -> Request:
        algo = self._coll_algo(algo)
        if algo == "window":
            req = self._coll_allgather(_flat(sendbuf), _flat(recvbuf), None, None, keep=(sendbuf, recvbuf))
            if req is not None:
                return req
        fb = "p2p" if algo == "p2p" else "auto"
        return self._bg(lambda: self.Allgather(sendbuf, recvbuf, algo=fb), keep=(sendbuf, recvbuf))

    def Ialltoall(self, sendbuf, recvbuf, algo: Optional[str] = None) -> Request:
        algo = self._coll_algo(algo)
        if algo == "window":
            req = self._coll_alltoall(_flat(sendbuf), _flat(recvbuf), keep=(sendbuf, recvbuf))
            if req is not None:
                return req
        fb = "p2p" if algo == "p2p" else "auto"
        return self._bg(lambda: self.Alltoall(sendbuf, recvbuf, algo=fb), keep=(sendbuf, recvbuf))

    @_pair_call
    def Ireduce_scatter(self, sendbuf, recvbuf, recvcounts=None, op=SUM, algo: Optional[str] = None,
                        pairtype=None) -> Request:
        algo = self._coll_algo(algo)
        if algo == "window":
            req = self._coll_reduce_scatter(_flat(sendbuf), _flat(recvbuf), recvcounts, op, keep=(sendbuf, recvbuf))
            if req is not None:
                return req
        fb = "p2p" if algo == "p2p" else "auto"
        return self._bg(lambda: self.Reduce_scatter(sendbuf, recvbuf, recvcounts, op, algo=fb),
                        keep=(sendbuf, recvbuf))

    def Gatherv(self, sendbuf, recvbuf, counts: Optional[Sequence[int]] = None, displs=None, root: int = 0,
                algo: Optional[str] = None):
        """``algo``: see "irregular window collectives" above (None: the MPIT_COLLECTIVES variable)."""
        n, me = self.Get_size(), self.Get_rank()
        src = _flat(sendbuf)
        if self._coll_algo(algo) == "window":
            req = self._vcoll_gatherv(src, recvbuf, counts, displs, root, keep=(sendbuf, recvbuf))
            if req is not None:
                req.Wait()
                return recvbuf
        if me != root:
            self._csend(src, root, 3).Wait()
            return recvbuf
        dst = _flat(recvbuf)
        if counts is None:
            counts = [src.numel()] * n
        if displs is None:
            displs = [sum(counts[:i]) for i in range(n)]
        reqs = []
        for q in range(n):
            seg = dst[displs[q]: displs[q] + counts[q]]
            if q == me:
                seg.copy_(src[: counts[q]])
            else:
                reqs.append(self._crecv(seg, q, 3))
        Request.Waitall(reqs)
        return recvbuf

    def Gather(self, sendbuf, recvbuf, root: int = 0, algo: Optional[str] = None):
        return self.Gatherv(sendbuf, recvbuf, None, None, root, algo=algo)

    def Scatterv(self, sendbuf, recvbuf, counts: Optional[Sequence[int]] = None, displs=None, root: int = 0,
                 algo: Optional[str] = None):
        """``algo``: see "irregular window collectives" above (None: the MPIT_COLLECTIVES variable)."""
        n, me = self.Get_size(), self.Get_rank()
        dst = _flat(recvbuf)
        if self._coll_algo(algo) == "window":
            req = self._vcoll_scatterv(sendbuf, dst, counts, displs, root, keep=(sendbuf, recvbuf))
            if req is not None:
                req.Wait()
                return recvbuf
        if me != root:
            self._crecv(dst, root, 4).Wait()
            return recvbuf
        src = _flat(sendbuf)
        if counts is None:
            counts = [dst.numel()] * n
        if displs is None:
            displs = [sum(counts[:i]) for i in range(n)]
        reqs = []
        for q in range(n):
            seg = src[displs[q]: displs[q] + counts[q]]
            if q == me:
                dst[: counts[q]].copy_(seg)
            else:
                reqs.append(self._csend(seg.contiguous(), q, 4))
        Request.Waitall(reqs)
        return recvbuf

    def Scatter(self, sendbuf, recvbuf, root: int = 0, algo: Optional[str] = None):
        return self.Scatterv(sendbuf, recvbuf, None, None, root, algo=algo)

    def Allgatherv(self, sendbuf, recvbuf, counts: Optional[Sequence[int]] = None, displs=None,
                   algo: Optional[str] = None):
        """``algo``: see "window collectives" above (None: the MPIT_COLLECTIVES variable)."""
        n = self.Get_size()
        src = _flat(sendbuf)
        dst = _flat(recvbuf)
        algo = self._coll_algo(algo)
        if algo == "window":
            req = self._coll_allgather(src, dst, counts, displs, keep=(sendbuf, recvbuf))
            if req is not None:
                req.Wait()
                return recvbuf
        if counts is None and algo != "p2p" and self._use_rccl(src):
            import torch.distributed as dist

            dist.all_gather_into_tensor(dst, src, group=self._pg)
            return recvbuf
        if counts is None:
            counts = [src.numel()] * n
        if displs is None:
            displs = [sum(counts[:i]) for i in range(n)]
        self.Gatherv(src, dst, counts, displs, 0, algo="auto")
        self.Bcast(dst, 0, algo="auto")
        return recvbuf

    def Allgather(self, sendbuf, recvbuf, algo: Optional[str] = None):
        return self.Allgatherv(sendbuf, recvbuf, None, None, algo=algo)

    def Alltoallv(self, sendbuf, sendcounts, sdispls, recvbuf, recvcounts, rdispls, algo: Optional[str] = None):
        """``algo``: see "irregular window collectives" above (None: the MPIT_COLLECTIVES variable)."""
        n, me = self.Get_size(), self.Get_rank()
        src, dst = _flat(sendbuf), _flat(recvbuf)
        if self._coll_algo(algo) == "window":
            req = self._vcoll_alltoallv(src, sendcounts, sdispls, dst, recvcounts, rdispls, keep=(sendbuf, recvbuf))
            if req is not None:
                req.Wait()
                return recvbuf
        reqs = []
        for q in range(n):
            rseg = dst[rdispls[q]: rdispls[q] + recvcounts[q]]
            sseg = src[sdispls[q]: sdispls[q] + sendcounts[q]]
            if q == me:
                rseg.copy_(sseg)
            else:
                reqs.append(self._crecv(rseg, q, 5))
                reqs.append(self._csend(sseg.contiguous(), q, 5))
        Request.Waitall(reqs)
        return recvbuf

    def Alltoall(self, sendbuf, recvbuf, algo: Optional[str] = None):
        """``algo``: see "window collectives" above (None: the MPIT_COLLECTIVES variable)."""
        n = self.Get_size()
        src, dst = _flat(sendbuf), _flat(recvbuf)
        algo = self._coll_algo(algo)
        if algo == "window":
            req = self._coll_alltoall(src, dst, keep=(sendbuf, recvbuf))
            if req is not None:
                req.Wait()
                return recvbuf
        if algo != "p2p" and self._use_rccl(src):
            import torch.distributed as dist

            dist.all_to_all_single(dst, src, group=self._pg)
            return recvbuf
        c = src.numel() // n
        d = [i * c for i in range(n)]
        return self.Alltoallv(src, [c] * n, d, dst, [c] * n, d, algo="auto")

    def Alltoallw(self, sendbufs: Sequence[torch.Tensor], recvbufs: Sequence[torch.Tensor],
                  algo: Optional[str] = None):
        """Per-peer tensors of arbitrary dtype/shape (MPI_Alltoallw's per-peer types). ``algo``: see
        "irregular window collectives" above (None: the MPIT_COLLECTIVES variable); by window the
        tensors may have any strides within three loops and are moved layout to layout."""
        n, me = self.Get_size(), self.Get_rank()
        if self._coll_algo(algo) == "window":
            req = self._vcoll("alltoallw", list(sendbufs), list(recvbufs), 0, keep=(sendbufs, recvbufs))
            if req is not None:
                req.Wait()
                return recvbufs
        reqs = []
        for q in range(n):
            if q == me:
                recvbufs[q].copy_(sendbufs[q])
            else:
                reqs.append(self._crecv(recvbufs[q], q, 6))
                reqs.append(self._csend(sendbufs[q].contiguous(), q, 6))
        Request.Waitall(reqs)
        return recvbufs

    @_pair_call
    def Reduce_scatter(self, sendbuf, recvbuf, recvcounts: Optional[Sequence[int]] = None, op: Op = SUM,
                       algo: Optional[str] = None, pairtype=None):
        """``algo``: see "window collectives" above (None: the MPIT_COLLECTIVES variable)."""
        n = self.Get_size()
        src, dst = _flat(sendbuf), _flat(recvbuf)
        if recvcounts is None:
            recvcounts = [src.numel() // n] * n
        algo = self._coll_algo(algo)
        if algo == "window":
            req = self._coll_reduce_scatter(src, dst, recvcounts, op, keep=(sendbuf, recvbuf))
            if req is not None:
                req.Wait()
                return recvbuf
        if algo != "p2p" and self._use_rccl(src) and _rccl_op(op) is not None and len(set(recvcounts)) == 1:
            import torch.distributed as dist

            dist.reduce_scatter_tensor(dst[: recvcounts[0]], src[: recvcounts[0] * n].contiguous(),
                                       op=_rccl_op(op), group=self._pg)
            return recvbuf
        tmp = torch.empty_like(src) if self.Get_rank() == 0 else None
        self.Reduce(src, tmp if tmp is not None else src, op, 0, algo="auto")
        displs = [sum(recvcounts[:i]) for i in range(n)]
        self.Scatterv(tmp, dst, recvcounts, displs, 0, algo="auto")
        return recvbuf

    @_pair_call
    def Reduce_scatter_block(self, sendbuf, recvbuf, op: Op = SUM, algo: Optional[str] = None, pairtype=None):
        return self.Reduce_scatter(sendbuf, recvbuf, None, op, algo=algo)

    @_pair_call
    def Scan(self, sendbuf, recvbuf, op: Op = SUM, algo: Optional[str] = None, pairtype=None):
        """Inclusive prefix reduction (linear chain, order-preserving). ``algo``: see "window
        collectives" above (None: the MPIT_COLLECTIVES variable)."""
        n, me = self.Get_size(), self.Get_rank()
        src, dst = _flat(sendbuf), _flat(recvbuf)
        if self._coll_algo(algo) == "window":
            req = self._coll_scan(src, dst, op, False, keep=(sendbuf, recvbuf))
            if req is not None:
                req.Wait()
                return recvbuf
        acc = src.clone()
        if me > 0:
            prev = torch.empty_like(src)
            self._crecv(prev, me - 1, 8).Wait()
            acc = op(prev, acc)
        if me < n - 1:
            self._csend(acc, me + 1, 8).Wait()
        dst.copy_(acc)
        return recvbuf

    @_pair_call
    def Exscan(self, sendbuf, recvbuf, op: Op = SUM, algo: Optional[str] = None, pairtype=None):
        """Exclusive prefix reduction; rank 0's recvbuf is left untouched (MPI). ``algo``: see
        "window collectives" above (None: the MPIT_COLLECTIVES variable)."""
        n, me = self.Get_size(), self.Get_rank()
        src, dst = _flat(sendbuf), _flat(recvbuf)
        if self._coll_algo(algo) == "window":
            req = self._coll_scan(src, dst, op, True, keep=(sendbuf, recvbuf))
            if req is not None:
                req.Wait()
                return recvbuf
        if me > 0:
            prev = torch.empty_like(src)
            self._crecv(prev, me - 1, 9).Wait()
            out = prev.clone()
            acc = op(prev, src)
        else:
            out = None
            acc = src.clone()
        if me < n - 1:
            self._csend(acc, me + 1, 9).Wait()
        if out is not None:
            dst.copy_(out)
        return recvbuf

    # object collectives (host, small)
    def allgather_obj(self, obj) -> list:
        import pickle

        data = torch.frombuffer(bytearray(pickle.dumps(obj)), dtype=torch.uint8)
        n = torch.tensor([data.numel()], dtype=torch.int64)
        sizes = torch.zeros(self.Get_size(), dtype=torch.int64)
        self.Allgather(n, sizes, algo="auto")
        buf = torch.zeros(int(sizes.sum()), dtype=torch.uint8)
        self.Allgatherv(data, buf, sizes.tolist(), algo="auto")
        out, o = [], 0
        for s in sizes.tolist():
            out.append(pickle.loads(buf[o: o + s].numpy().tobytes()))
            o += s
        return out

    def bcast_obj(self, obj, root=0):
        return self.allgather_obj(obj if self.Get_rank() == root else None)[root]

    # ---------------------------------------------------------------- constructors
    def _agree_ctx(self) -> int:
        """Collectively agree on a fresh context id (max of the members' counters)."""
        st = _rt.state()
        mine = torch.tensor([st.next_ctx], dtype=torch.int64)
        out = torch.zeros(1, dtype=torch.int64)
        self.Allreduce(mine, out, MAX, algo="auto")  # (creating a window agrees on a context: never through one)
        ctx = int(out.item())
        st.next_ctx = ctx + 1
        return ctx * 2  # even: user p2p; ctx + 2^20: collectives

    def Dup(self) -> "Comm":
        c = Comm(self._ranks, self._agree_ctx(), self._name + "_dup")
        c._attrs = dict(self._attrs)
        return c

    Idup = Dup

    def Create(self, group) -> Optional["Comm"]:
        ctx = self._agree_ctx()
        if _rt.state().rank not in group.world_ranks:
            return None
        return Comm(group.world_ranks, ctx)

    def Split(self, color: int, key: int = 0) -> Optional["Comm"]:
        ctx = self._agree_ctx()
        entries = self.allgather_obj((color, key, _rt.state().rank))
        if color == UNDEFINED:
            return None
        mine = sorted([(k, w) for (c, k, w) in entries if c == color])
        colors = sorted({c for (c, _, _) in entries if c != UNDEFINED})
        return Comm([w for (_, w) in mine], ctx + 2 * _COLL_OFFSET * (1 + colors.index(color)))

    def Compare(self, other: "Comm") -> int:
        if other is self:
            return IDENT
        if self._ranks == other._ranks:
            return CONGRUENT
        if sorted(self._ranks) == sorted(other._ranks):
            return SIMILAR
        return UNEQUAL

    def Free(self):
        self._pg = None
        self._ar_stop()  # (drains the FIFO: no member is inside an all-reduce of ours after it)
        for rec in self._sym:  # symmetric memory still registered, the staging buffers included
            rec.win.Free()
        self._sym, self._ar_stage = [], {}

    def Disconnect(self):
        self.Barrier()
        self.Free()

    def Abort(self, code: int = 1):
        _rt.Abort(code)

    def __repr__(self):
        return f"Comm(name={self._name!r}, rank={self.Get_rank()}, size={self.Get_size()})"


COMM_NULL = None
_world: Optional[Comm] = None
_self: Optional[Comm] = None


def COMM_WORLD() -> Comm:
    global _world
    st = _rt.state()
    if _world is None or _world._ranks != list(range(st.world)):
        _world = Comm(list(range(st.world)), 0, "MPI_COMM_WORLD")
    return _world


def COMM_SELF() -> Comm:
    global _self
    st = _rt.state()
    if _self is None or _self._ranks != [st.rank]:
        _self = Comm([st.rank], 2, "MPI_COMM_SELF")
    return _self


def _reset_singletons():
    global _world, _self
    _world = None
    _self = None
