"""MPI datatypes: the 22 basic types of the reference (lua-mpi.h:130-151) and derived
type constructors (mpifuncs.c Type_* / Pack* wrappers, SURVEY Appendix A "Datatypes").

A :class:`Datatype` is a *typemap*: a list of (byte displacement, basic type) plus lower
bound and extent. ``pack`` / ``unpack`` move ``count`` instances between a tensor (viewed
as bytes) and a contiguous byte stream in one launch of the type_copy kernel
(csrc/kernels/type_copy.hip; its host twin for host tensors) driven by a compact layout
:class:`Plan` (loops around a run table, built once per type). The byte-index gather /
scatter remains as the fallback: ``MPIT_DTYPE_KERNEL=0``, a negative displacement, or a
native module that does not load. Either way the layout's last byte is checked against the
buffer on the host first (``IndexError``). ``layout_of`` gives the same kind of plan for a
non-contiguous tensor, which lets point-to-point calls send and receive strided views.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

# which path moved the bytes: `kernel` = type_copy launches (pack / unpack / send / recv and
# the packing of a derived one-sided origin), `index` = the byte-index fallback, `rma_kernel` =
# one-launch Put / Get on a derived target type, `rma_copies` = per-run peer copies,
# `rma_acc_kernel` = one-launch Accumulate / Get_accumulate calls (type_accumulate),
# `rma_acc_runs` = per-run axpby accumulates of the fallback path
COUNTERS = {"kernel": 0, "index": 0, "rma_kernel": 0, "rma_copies": 0, "rma_acc_kernel": 0, "rma_acc_runs": 0}

_BASIC: Dict[str, Tuple[int, Optional[torch.dtype]]] = {
    "CHAR": (1, torch.int8), "BYTE": (1, torch.uint8), "SHORT": (2, torch.int16), "INT": (4, torch.int32),
    "LONG": (8, torch.int64), "FLOAT": (4, torch.float32), "DOUBLE": (8, torch.float64),
    "UNSIGNED_CHAR": (1, torch.uint8), "UNSIGNED_SHORT": (2, torch.int16), "UNSIGNED": (4, torch.int32),
    "UNSIGNED_LONG": (8, torch.int64), "LONG_DOUBLE": (16, None), "LONG_LONG_INT": (8, torch.int64),
    "FLOAT_INT": (8, None), "LONG_INT": (16, None), "DOUBLE_INT": (16, None), "SHORT_INT": (8, None),
    "2INT": (8, None), "LONG_DOUBLE_INT": (32, None), "PACKED": (1, torch.uint8), "UB": (0, None), "LB": (0, None),
    "BFLOAT16": (2, torch.bfloat16), "HALF": (2, torch.float16), "BOOL": (1, torch.bool),
}


# -------------------------------------------------------------------- layout plans

def _low_bit(x: int) -> int:
    """The largest power of two <= 16 that divides x (16 for 0)."""
    x = int(x) & 15
    return (x & -x) if x else 16


def _fold_once(offs: np.ndarray, lens: np.ndarray):
    """offs / lens of R runs -> ((n, stride), offs[:p], lens[:p]) for the smallest period p < R
    with lens[i + p] == lens[i] and offs[i + p] == offs[i] + stride, or None. One vectorised
    comparison per divisor of R."""
    R = len(offs)
    small = [p for p in range(1, int(R ** 0.5) + 1) if R % p == 0]
    for p in sorted(set(small + [R // p for p in small])):
        if p == R or lens[p] != lens[0]:
            continue
        d = int(offs[p] - offs[0])
        if np.array_equal(lens[p:], lens[:-p]) and bool((offs[p:] - offs[:-p] == d).all()):
            return (R // p, d), offs[:p], lens[:p]
    return None


class Plan:
    """`loops` around a run table, the layout type_copy (csrc/kernels/type_copy.hip) walks.

    loops: up to three (n, stride bytes) with n > 1, outermost first; offs / lens: the R runs
    (byte offset, length > 0) in packed order; prefix: the R + 1 prefix sums of lens; L: the
    common run length or 0; per = prefix[R]; total: the packed bytes; [lo, hi): the bytes
    touched relative to the base address (hi == lo == 0 for an empty plan); align: the largest
    power of two <= 16 dividing every offset, length and stride. Packed order: loops outermost
    to innermost, runs in table order, ascending bytes."""

    def __init__(self, loops, offs: np.ndarray, lens: np.ndarray, tables: Optional[dict] = None):
        self.loops = tuple((int(n), int(s)) for n, s in loops)
        if len(self.loops) > 3:
            raise ValueError("a layout plan holds at most three loops")
        self.offs, self.lens = offs, lens
        self.R = len(offs)
        self.prefix = np.zeros(self.R + 1, dtype=np.int64)
        np.cumsum(lens, out=self.prefix[1:])
        self.per = int(self.prefix[-1])
        iters = 1
        for n, _ in self.loops:
            iters *= n
        self.total = iters * self.per
        if self.total == 0:
            self.L = self.lo = self.hi = 0
            self.align = 16
        else:
            self.L = int(lens[0]) if bool((lens == lens[0]).all()) else 0
            self.lo, self.hi = int(offs.min()), int((offs + lens).max())
            bits = int(np.bitwise_or.reduce(offs | lens))
            for n, s in self.loops:
                self.lo += min(0, (n - 1) * s)
                self.hi += max(0, (n - 1) * s)
                bits |= s
            self.align = _low_bit(bits)
        self._tables = tables if tables is not None else {}  # device -> uploaded [offs | prefix]
        self._off0 = int(offs[0]) if self.R == 1 else 0
        self._loops = [list(x) for x in self.loops]  # as the binding takes them

    def unit(self, strided_addr: int, packed_addr: int) -> int:
        """Bytes a lane moves per access between these two base addresses."""
        bits = self.align | strided_addr | packed_addr  # align <= 16 bounds the lowest set bit
        return bits & -bits

    def table(self, device) -> Tuple[int, int, Optional[torch.Tensor]]:
        """(table address, byte offset to add to the strided base, the tensor to keep alive). One
        run needs no table: its offset moves into the base. Otherwise int64 [offs | prefix],
        uploaded once per device with a host-blocking copy (complete on return, so any stream
        may read it) and cached."""
        if self.R == 1:
            return 0, self._off0, None
        t = self._tables.get(device)
        if t is None:
            t = torch.from_numpy(np.concatenate([self.offs, self.prefix])).to(device, non_blocking=False)
            self._tables[device] = t
        return t.data_ptr(), 0, t

    def self_overlap(self) -> bool:
        """True when a one-run plan's loops may write a byte twice (a zero or overlapping stride)."""
        span = self.L
        for n, s in sorted(self.loops, key=lambda ns: abs(ns[1])):
            if abs(s) < span:
                return True
            span += (n - 1) * abs(s)
        return False

    def __repr__(self):
        return f"Plan(loops={self.loops}, R={self.R}, L={self.L}, total={self.total}, span=[{self.lo}, {self.hi}))"


_native_ok: Optional[bool] = None


def kernel_enabled() -> bool:
    """type_copy moves the bytes unless MPIT_DTYPE_KERNEL=0 or the native module does not load."""
    global _native_ok
    if os.environ.get("MPIT_DTYPE_KERNEL", "1") == "0":
        return False
    if _native_ok is None:
        try:
            from ._ext import native

            native()
            _native_ok = True
        except Exception:
            _native_ok = False
    return _native_ok


_nat = None


def run_plan(plan: Plan, direction: int, strided: torch.Tensor, packed: torch.Tensor, max_blocks: int = 0,
             wide: bool = False):
    """One type_copy launch (the host twin for CPU tensors): direction 0 gathers the plan's bytes
    at `strided`'s first byte into `packed`, 1 scatters. The caller has checked the plan's span
    against the strided buffer and that `packed` is contiguous, on the same device and holds
    plan.total bytes. Kept short: at small sizes a call costs what this function costs."""
    global _nat
    if plan.total == 0:
        return
    if _nat is None:
        from ._ext import native

        _nat = native()
    dev, stream = -1, 0
    if strided.is_cuda:
        dev = strided.device.index
        stream = torch._C._cuda_getCurrentRawStream(dev)
    tab, off, _keep = plan.table(strided.device)
    sp, pp = strided.data_ptr() + off, packed.data_ptr()
    bits = plan.align | sp | pp
    _nat.type_copy(dev, stream, direction, sp, pp, plan._loops, tab, plan.R, plan.L, plan.per, bits & -bits,
                   max_blocks, wide)
    COUNTERS["kernel"] += 1


def layout_of(t: torch.Tensor) -> Plan:
    """The plan of a strided tensor's bytes in logical (row-major) order, relative to its
    data_ptr(): size-1 dims dropped, adjacent dims merged where the outer stride continues the
    inner one, a unit-stride innermost dim turned into the run. ValueError when more than three
    loops remain or an offset is negative."""
    es = t.element_size()
    dims = [(int(n), int(s) * es) for n, s in zip(t.shape, t.stride()) if n != 1]
    if any(n == 0 for n, _ in dims):
        return Plan((), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    if any(s < 0 for _, s in dims):
        raise ValueError("layout_of: negative strides (negative offsets) are not supported")
    merged: List[Tuple[int, int]] = []
    for n, s in dims:
        if merged and merged[-1][1] == n * s:
            merged[-1] = (merged[-1][0] * n, s)
        else:
            merged.append((n, s))
    run = es
    if merged and merged[-1][1] == es:
        run = merged.pop()[0] * es
    if len(merged) > 3:
        raise ValueError(f"layout_of: {len(merged)} strided loops remain after collapsing; more than three loops "
                         "are not supported (make the tensor contiguous first)")
    return Plan(merged, np.zeros(1, dtype=np.int64), np.array([run], dtype=np.int64))


def pack_tensor(t: torch.Tensor) -> torch.Tensor:
    """A non-contiguous tensor's elements in logical order as a new contiguous 1-D tensor."""
    out = torch.empty(t.numel(), dtype=t.dtype, device=t.device)
    if kernel_enabled():
        run_plan(layout_of(t), 0, _bytes_at(t), out.view(torch.uint8))
    else:
        COUNTERS["index"] += 1
        out.copy_(t.reshape(-1))
    return out


def unpack_tensor(packed: torch.Tensor, t: torch.Tensor):
    """Scatter a contiguous stream of t.numel() elements into the non-contiguous tensor `t`."""
    check_writable_layout(t)
    if packed.numel() != t.numel() or packed.dtype != t.dtype or packed.device != t.device:
        raise ValueError("unpack_tensor: the stream must hold t.numel() elements of t's dtype on t's device")
    if kernel_enabled():
        run_plan(layout_of(t), 1, _bytes_at(t), packed.contiguous().reshape(-1).view(torch.uint8))
    else:
        COUNTERS["index"] += 1
        t.copy_(packed.reshape(-1).view(t.dtype).reshape(t.shape))
    return t


def check_writable_layout(t: torch.Tensor):
    if layout_of(t).self_overlap():
        raise ValueError("cannot receive / unpack into a tensor with a zero or overlapping stride")


def _bytes_at(t: torch.Tensor) -> torch.Tensor:
    """A one-element uint8 tensor at t's first byte (the base address of its layout, kept alive by
    the storage it shares)."""
    return torch.as_strided(t, (1,), (1,)).view(torch.uint8)[:1] if t.numel() else t.reshape(-1).view(torch.uint8)


class Datatype:
    def __init__(self, typemap: List[Tuple[int, str]], lb: int, extent: int, name: str = "",
                 envelope=("NAMED", (), ()), committed=True):
        self.typemap = typemap  # [(disp_bytes, basic_name)]
        self.lb = lb
        self.extent = extent
        self._name = name
        self.envelope = envelope
        self.committed = committed
        self._attrs = {}
        self._idx_cache = {}
        self._fold_cache = None  # the folded instance layout (plan)
        self._plan_cache = {}  # count -> Plan
        self._tab_cache = {}  # device -> uploaded run table, shared by the plans of every count
        self._elem_cache = None  # (type-map length, element_dtype())

    # ---------------------------------------------------------------- queries
    def Get_size(self) -> int:
        return sum(_BASIC[b][0] for _, b in self.typemap)

    def Get_extent(self) -> Tuple[int, int]:
        return self.lb, self.extent

    def Get_true_extent(self) -> Tuple[int, int]:
        if not self.typemap:
            return 0, 0
        lo = min(d for d, _ in self.typemap)
        hi = max(d + _BASIC[b][0] for d, b in self.typemap)
        return lo, hi - lo

    def Get_envelope(self):
        kind, ints, types = self.envelope
        return len(ints), 0, len(types), kind

    def Get_contents(self):
        return self.envelope

    def Get_name(self) -> str:
        return self._name

    def Set_name(self, n: str):
        self._name = n

    def Commit(self):
        self.committed = True
        return self

    def Free(self):
        self._idx_cache.clear()
        self._plan_cache.clear()
        self._tab_cache.clear()

    def Dup(self) -> "Datatype":
        return Datatype(list(self.typemap), self.lb, self.extent, self._name, ("DUP", (), (self,)))

    def Set_attr(self, k, v):
        self._attrs[k] = v

    def Get_attr(self, k):
        return self._attrs.get(k)

    def Delete_attr(self, k):
        self._attrs.pop(k, None)

    def is_contiguous_basic(self) -> bool:
        return len(self.typemap) == 1 and self.typemap[0][0] == 0 and self.extent == _BASIC[self.typemap[0][1]][0]

    @property
    def torch_dtype(self) -> Optional[torch.dtype]:
        if len(self.typemap) == 1:
            return _BASIC[self.typemap[0][1]][1]
        return None

    # ---------------------------------------------------------------- byte gather / scatter
    def _byte_index(self, count: int, device) -> torch.Tensor:
        key = (count, str(device))
        t = self._idx_cache.get(key)
        if t is None:
            idx = []
            for i in range(count):
                base = i * self.extent
                for d, b in self.typemap:
                    sz = _BASIC[b][0]
                    idx.extend(range(base + d, base + d + sz))
            t = torch.tensor(idx, dtype=torch.int64, device=device)
            self._idx_cache[key] = t
        return t

    def _count_for(self, buf: torch.Tensor, count: Optional[int]) -> int:
        if count is not None:
            return int(count)
        nbytes = buf.numel() * buf.element_size()
        return max(0, (nbytes - self.Get_true_extent()[1]) // max(1, self.extent) + 1) if self.extent else 1

    # ---------------------------------------------------------------- layout plan
    def _folded(self):
        """(inner loops, offs, lens) of ONE instance: the merged runs of the type map, an
        arithmetic progression of equal-length runs folded into a loop (at most twice)."""
        if self._fold_cache is None:
            tm = [(d, _BASIC[b][0]) for d, b in self.typemap if _BASIC[b][0]]
            arr = np.array(tm, dtype=np.int64).reshape(-1, 2)
            offs, lens = arr[:, 0], arr[:, 1]
            if len(offs) > 1:  # merge adjacent entries, as runs() does
                first = np.concatenate([[True], offs[1:] != offs[:-1] + lens[:-1]])
                starts = np.flatnonzero(first)
                lens = np.add.reduceat(lens, starts)
                offs = offs[starts]
            loops = []
            while len(loops) < 2:
                f = _fold_once(offs, lens)
                if f is None:
                    break
                loops.append(f[0])
                offs, lens = f[1], f[2]
            self._fold_cache = (loops, np.ascontiguousarray(offs), np.ascontiguousarray(lens))
        return self._fold_cache

    def plan(self, count: int) -> Plan:
        """The layout of `count` instances (see :class:`Plan`): the folded instance under the
        loop (count, extent). Built once per type; a count costs nothing but the small object."""
        count = int(count)
        p = self._plan_cache.get(count)
        if p is None:
            loops, offs, lens = self._folded()
            loops = list(loops)
            if count <= 0 or not len(offs):
                p = Plan((), offs[:0], lens[:0])
            else:
                if count > 1:
                    if loops and loops[0][0] * loops[0][1] == self.extent:  # instances continue the outer loop
                        loops[0] = (loops[0][0] * count, loops[0][1])
                    elif not loops and len(offs) == 1 and int(lens[0]) == self.extent:  # contiguous instances
                        lens = lens * count
                    else:
                        loops.insert(0, (count, self.extent))
                tables = self._tab_cache if len(lens) > 1 else None
                p = Plan(loops, offs, lens, tables)
            self._plan_cache[count] = p
        return p

    def _check_span(self, plan: Plan, nbytes: int):
        """Host-side guard of both paths: the plan's bytes lie inside the buffer (a negative
        displacement may reach back at most the buffer's length: the index path wraps it)."""
        if plan.total and (plan.hi > nbytes or plan.lo < -nbytes):
            raise IndexError(f"{self!r}: bytes [{plan.lo}, {plan.hi}) of the layout lie outside a buffer of {nbytes} bytes")

    def pack(self, buf: torch.Tensor, count: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Gather `count` instances from `buf` into a contiguous uint8 tensor (`out`, when given:
        uint8, contiguous, on buf's device, exactly the packed size)."""
        if count is None:
            count = self._count_for(buf, None)
        plan = self._plan_cache.get(count) or self.plan(count)
        raw = buf if buf.is_contiguous() else buf.contiguous()
        nbytes = raw.numel() * raw.element_size()
        if plan.hi > nbytes or plan.lo < -nbytes:
            self._check_span(plan, nbytes)
        if out is not None and (out.dtype != torch.uint8 or out.numel() != plan.total or out.device != raw.device
                                or not out.is_contiguous()):
            raise ValueError("pack: `out` must be uint8, contiguous, on the buffer's device and of the packed size")
        if plan.lo < 0 or not kernel_enabled():
            COUNTERS["index"] += 1
            raw = raw.reshape(-1).view(torch.uint8)
            data = raw[self._byte_index(count, raw.device)]
            return data if out is None else out.copy_(data)
        if out is None:
            out = torch.empty(plan.total, dtype=torch.uint8, device=raw.device)
        run_plan(plan, 0, raw, out)
        return out

    def staging(self, buf: torch.Tensor, count: Optional[int] = None) -> torch.Tensor:
        count = self._count_for(buf, count)
        return torch.empty(count * self.Get_size(), dtype=torch.uint8, device=buf.device)

    def unpack(self, packed: torch.Tensor, buf: torch.Tensor, count: Optional[int] = None):
        """Scatter a packed byte stream into `buf` (in place)."""
        if count is None:
            count = self._count_for(buf, None)
        if not buf.is_contiguous():
            raise ValueError("unpack target must be contiguous")
        plan = self._plan_cache.get(count) or self.plan(count)
        nbytes = buf.numel() * buf.element_size()
        if plan.hi > nbytes or plan.lo < -nbytes:
            self._check_span(plan, nbytes)
        if plan.lo < 0 or not kernel_enabled():
            COUNTERS["index"] += 1
            raw = buf.reshape(-1).view(torch.uint8)
            raw[self._byte_index(count, raw.device)] = packed.reshape(-1)[: count * self.Get_size()].to(raw.device)
            return buf
        src = packed
        if src.dtype != torch.uint8 or src.dim() != 1 or src.device != buf.device or not src.is_contiguous():
            src = packed.reshape(-1)
            if src.dtype != torch.uint8:
                src = src.contiguous().view(torch.uint8)
            src = src.to(buf.device).contiguous()
        if src.numel() < plan.total:
            raise ValueError(f"unpack: the packed stream holds {src.numel()} bytes, {count} x {self!r} needs {plan.total}")
        run_plan(plan, 1, buf, src)
        return buf

    def runs(self, count: int) -> List[Tuple[int, int]]:
        """The byte runs (offset, length) that `count` instances occupy, in type-map order
        (the order of the packed stream), adjacent segments merged: what a one-sided
        transfer moves with one copy each."""
        out: List[Tuple[int, int]] = []
        for i in range(int(count)):
            base = i * self.extent
            for d, b in self.typemap:
                sz = _BASIC[b][0]
                if not sz:
                    continue
                o = base + d
                if out and out[-1][0] + out[-1][1] == o:
                    out[-1] = (out[-1][0], out[-1][1] + sz)
                else:
                    out.append((o, sz))
        return out

    def element_dtype(self) -> Optional[torch.dtype]:
        """The one basic torch dtype every entry of the type map has (None: mixed / none)."""
        key = len(self.typemap)  # walked once per type, not once per one-sided call
        if self._elem_cache is None or self._elem_cache[0] != key:
            kinds = {b for _, b in self.typemap if _BASIC[b][0]}
            self._elem_cache = (key, _BASIC[kinds.pop()][1] if len(kinds) == 1 else None)
        return self._elem_cache[1]

    def __repr__(self):
        return f"Datatype({self._name or self.envelope[0]}, size={self.Get_size()}, extent={self.extent})"


def _basic(name: str) -> Datatype:
    sz = _BASIC[name][0]
    return Datatype([(0, name)] if sz else [], 0, sz, "MPI_" + name)


CHAR, BYTE, SHORT, INT, LONG, FLOAT, DOUBLE = (_basic(n) for n in ("CHAR", "BYTE", "SHORT", "INT", "LONG", "FLOAT", "DOUBLE"))
UNSIGNED_CHAR, UNSIGNED_SHORT, UNSIGNED, UNSIGNED_LONG = (_basic(n) for n in ("UNSIGNED_CHAR", "UNSIGNED_SHORT", "UNSIGNED", "UNSIGNED_LONG"))
LONG_DOUBLE, LONG_LONG_INT, PACKED, UB, LB = (_basic(n) for n in ("LONG_DOUBLE", "LONG_LONG_INT", "PACKED", "UB", "LB"))
BFLOAT16, HALF, BOOL = _basic("BFLOAT16"), _basic("HALF"), _basic("BOOL")


def _pair(vname: str, iname: str, name: str) -> Datatype:
    vs, is_ = _BASIC[vname][0], _BASIC[iname][0]
    al = max(vs, is_)
    ext = (vs + is_ + al - 1) // al * al
    return Datatype([(0, vname), (vs, iname)], 0, ext, name)


FLOAT_INT = _pair("FLOAT", "INT", "MPI_FLOAT_INT")
DOUBLE_INT = _pair("DOUBLE", "INT", "MPI_DOUBLE_INT")
LONG_INT = _pair("LONG", "INT", "MPI_LONG_INT")
SHORT_INT = _pair("SHORT", "INT", "MPI_SHORT_INT")
TWOINT = _pair("INT", "INT", "MPI_2INT")
LONG_DOUBLE_INT = Datatype([(0, "LONG_DOUBLE"), (16, "INT")], 0, 32, "MPI_LONG_DOUBLE_INT")
DATATYPE_NULL = None

_BY_TORCH = {torch.float32: FLOAT, torch.float64: DOUBLE, torch.int32: INT, torch.int64: LONG, torch.int16: SHORT,
             torch.int8: CHAR, torch.uint8: BYTE, torch.bfloat16: BFLOAT16, torch.float16: HALF, torch.bool: BOOL}


def from_torch(dtype: torch.dtype) -> Datatype:
    return _BY_TORCH[dtype]


# -------------------------------------------------------------------- constructors

def _concat(parts: List[Tuple[int, Datatype, int]]) -> List[Tuple[int, str]]:
    """parts: (byte displacement, type, count) -> flattened typemap."""
    tm = []
    for disp, t, cnt in parts:
        for i in range(cnt):
            base = disp + i * t.extent
            tm.extend((base + d, b) for d, b in t.typemap)
    return tm


def _bounds(tm, lb=None, ub=None):
    if not tm:
        return 0, 0
    lo = min(d for d, _ in tm) if lb is None else lb
    hi = max(d + _BASIC[b][0] for d, b in tm) if ub is None else ub
    return lo, hi - lo


def Type_contiguous(count: int, oldtype: Datatype) -> Datatype:
    tm = _concat([(0, oldtype, count)])
    return Datatype(tm, oldtype.lb, count * oldtype.extent, envelope=("CONTIGUOUS", (count,), (oldtype,)), committed=False)


def Type_vector(count: int, blocklength: int, stride: int, oldtype: Datatype) -> Datatype:
    return Type_create_hvector(count, blocklength, stride * oldtype.extent, oldtype, _kind="VECTOR")


def Type_create_hvector(count: int, blocklength: int, stride_bytes: int, oldtype: Datatype, _kind="HVECTOR") -> Datatype:
    tm = _concat([(i * stride_bytes, oldtype, blocklength) for i in range(count)])
    lb, ext = _bounds(tm)
    ext = (count - 1) * stride_bytes + blocklength * oldtype.extent if count else 0
    return Datatype(tm, 0, ext, envelope=(_kind, (count, blocklength, stride_bytes), (oldtype,)), committed=False)


def Type_indexed(blocklengths: Sequence[int], displacements: Sequence[int], oldtype: Datatype) -> Datatype:
    return Type_create_hindexed(blocklengths, [d * oldtype.extent for d in displacements], oldtype, _kind="INDEXED")


def Type_create_hindexed(blocklengths, displacements_bytes, oldtype: Datatype, _kind="HINDEXED") -> Datatype:
    tm = _concat([(d, oldtype, b) for b, d in zip(blocklengths, displacements_bytes)])
    ends = [d + b * oldtype.extent for b, d in zip(blocklengths, displacements_bytes)]
    lb = min(displacements_bytes) if displacements_bytes else 0
    ext = (max(ends) - lb) if ends else 0
    return Datatype(tm, lb, ext, envelope=(_kind, (tuple(blocklengths), tuple(displacements_bytes)), (oldtype,)),
                    committed=False)


def Type_create_indexed_block(blocklength: int, displacements: Sequence[int], oldtype: Datatype) -> Datatype:
    return Type_indexed([blocklength] * len(displacements), displacements, oldtype)


def Type_create_struct(blocklengths, displacements_bytes, types: Sequence[Datatype]) -> Datatype:
    tm = _concat([(d, t, b) for b, d, t in zip(blocklengths, displacements_bytes, types)])
    ends = [d + b * t.extent for b, d, t in zip(blocklengths, displacements_bytes, types)]
    lb = min(displacements_bytes) if displacements_bytes else 0
    ext = (max(ends) - lb) if ends else 0
    return Datatype(tm, lb, ext, envelope=("STRUCT", (tuple(blocklengths), tuple(displacements_bytes)), tuple(types)),
                    committed=False)


ORDER_C, ORDER_FORTRAN = 56, 57


def Type_create_subarray(sizes, subsizes, starts, order: int, oldtype: Datatype) -> Datatype:
    import itertools

    nd = len(sizes)
    # element strides: row-major (last dim fastest) for C, column-major for Fortran
    fastest_last = order == ORDER_C
    strides, s = [0] * nd, oldtype.extent
    for d in (reversed(range(nd)) if fastest_last else range(nd)):
        strides[d] = s
        s *= sizes[d]
    total = s
    tm = []
    for idx in itertools.product(*[range(starts[d], starts[d] + subsizes[d]) for d in range(nd)]):
        off = sum(i * st for i, st in zip(idx, strides))
        tm.append((off, idx))
    tm.sort()
    tm = [(off + dd, b) for off, _ in tm for dd, b in oldtype.typemap]
    return Datatype(tm, 0, total, envelope=("SUBARRAY", (tuple(sizes), tuple(subsizes), tuple(starts), order), (oldtype,)),
                    committed=False)


DISTRIBUTE_BLOCK, DISTRIBUTE_CYCLIC, DISTRIBUTE_NONE, DISTRIBUTE_DFLT_DARG = 121, 122, 123, -49767


def Type_create_darray(size, rank, gsizes, distribs, dargs, psizes, order, oldtype) -> Datatype:
    """Block (and block-cyclic) distribution of a global array over a process grid."""
    # process coordinates in row-major order of psizes
    coords, r = [], rank
    for p in reversed(psizes):
        coords.append(r % p)
        r //= p
    coords = coords[::-1]
    ranges = []
    for d, g in enumerate(gsizes):
        p, c = psizes[d], coords[d]
        if distribs[d] == DISTRIBUTE_NONE or p == 1:
            ranges.append(list(range(g)))
        elif distribs[d] == DISTRIBUTE_BLOCK:
            b = dargs[d] if dargs[d] not in (DISTRIBUTE_DFLT_DARG, 0) else -(-g // p)
            ranges.append(list(range(c * b, min(g, (c + 1) * b))))
        else:  # cyclic(b)
            b = dargs[d] if dargs[d] not in (DISTRIBUTE_DFLT_DARG, 0) else 1
            ranges.append([i for i in range(g) if (i // b) % p == c])
    import itertools

    strides, s = [0] * len(gsizes), oldtype.extent
    for d in reversed(range(len(gsizes))):
        strides[d] = s
        s *= gsizes[d]
    tm = []
    for idx in itertools.product(*ranges):
        off = sum(i * st for i, st in zip(idx, strides))
        tm.extend((off + dd, b) for dd, b in oldtype.typemap)
    return Datatype(tm, 0, s, envelope=("DARRAY", (size, rank, tuple(gsizes)), (oldtype,)), committed=False)


def Type_create_resized(oldtype: Datatype, lb: int, extent: int) -> Datatype:
    return Datatype(list(oldtype.typemap), lb, extent, envelope=("RESIZED", (lb, extent), (oldtype,)), committed=False)


def Type_dup(t: Datatype) -> Datatype:
    return t.Dup()


def Type_commit(t: Datatype) -> Datatype:
    return t.Commit()


def Type_free(t: Datatype):
    t.Free()


def Type_size(t: Datatype) -> int:
    return t.Get_size()


def Type_get_extent(t: Datatype):
    return t.Get_extent()


def Type_get_true_extent(t: Datatype):
    return t.Get_true_extent()


def Type_get_envelope(t: Datatype):
    return t.Get_envelope()


def Type_get_contents(t: Datatype):
    return t.Get_contents()


def Type_get_name(t: Datatype) -> str:
    return t.Get_name()


def Type_set_name(t: Datatype, name: str):
    t.Set_name(name)


TYPECLASS_INTEGER, TYPECLASS_REAL, TYPECLASS_COMPLEX = 1, 2, 3


def Type_match_size(typeclass: int, size: int) -> Datatype:
    table = {TYPECLASS_INTEGER: {1: CHAR, 2: SHORT, 4: INT, 8: LONG}, TYPECLASS_REAL: {2: HALF, 4: FLOAT, 8: DOUBLE}}
    try:
        return table[typeclass][size]
    except KeyError:
        raise ValueError(f"no datatype of class {typeclass} and size {size}") from None


# -------------------------------------------------------------------- Pack / Unpack

def Pack(inbuf: torch.Tensor, incount: int, datatype: Datatype, outbuf: torch.Tensor, position: int) -> int:
    """Append `incount` instances to the byte buffer `outbuf` at `position`; returns the
    new position (MPI_Pack)."""
    out = outbuf.reshape(-1).view(torch.uint8)
    n = int(incount) * datatype.Get_size()
    if outbuf.is_contiguous() and out.device == inbuf.device and 0 <= position and position + n <= out.numel():
        datatype.pack(inbuf, incount, out=out[position: position + n])  # straight into place
        return position + n
    data = datatype.pack(inbuf, incount)
    out[position: position + data.numel()] = data.to(out.device)
    return position + data.numel()


def Unpack(inbuf: torch.Tensor, position: int, outbuf: torch.Tensor, outcount: int, datatype: Datatype) -> int:
    src = inbuf.reshape(-1).view(torch.uint8)
    n = outcount * datatype.Get_size()
    datatype.unpack(src[position: position + n], outbuf, outcount)
    return position + n


def Pack_size(incount: int, datatype: Datatype) -> int:
    return incount * datatype.Get_size()


def Pack_external(datarep: str, inbuf, incount, datatype, outbuf, position) -> int:
    """"external32" = big-endian canonical representation."""
    if datarep not in ("external32", "native"):
        raise ValueError("supported data representations: external32, native")
    pos0 = position
    position = Pack(inbuf, incount, datatype, outbuf, position)
    if datarep == "external32":
        _byteswap_inplace(outbuf.reshape(-1).view(torch.uint8)[pos0:position], datatype, incount)
    return position


def Unpack_external(datarep: str, inbuf, position, outbuf, outcount, datatype) -> int:
    src = inbuf.reshape(-1).view(torch.uint8)
    n = outcount * datatype.Get_size()
    seg = src[position: position + n].clone()
    if datarep == "external32":
        _byteswap_inplace(seg, datatype, outcount)
    datatype.unpack(seg, outbuf, outcount)
    return position + n


def Pack_external_size(datarep: str, incount: int, datatype: Datatype) -> int:
    return Pack_size(incount, datatype)


def _byteswap_inplace(seg: torch.Tensor, datatype: Datatype, count: int):
    o = 0
    for _ in range(count):
        for _, b in datatype.typemap:
            sz = _BASIC[b][0]
            if sz > 1:
                seg[o: o + sz] = seg[o: o + sz].flip(0)
            o += sz


def Get_address(t: torch.Tensor) -> int:
    return t.data_ptr()


def Get_elements(status, datatype: Datatype) -> int:
    """Number of basic elements received."""
    per = len(datatype.typemap) or 1
    return (status.count // max(1, datatype.Get_size())) * per


_datareps = {}


def Register_datarep(name: str, read_fn, write_fn, extent_fn, extra_state=None):
    _datareps[name] = (read_fn, write_fn, extent_fn, extra_state)
