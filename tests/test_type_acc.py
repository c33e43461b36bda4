"""One-sided accumulate in one launch: the type_accumulate kernel and its host twin
(csrc/kernels/type_acc.hip) through the raw binding, in one process.

The oracle is independent of the code under test. The layout comes from the type map's
definition (instance i of a type places the bytes of entry (d, basic) at i * extent + d), never
from Datatype.pack. The value is comb(target, origin) as csrc/kernels/kernels.h defines it,
computed in torch / numpy on the host: bf16 / fp16 widen to fp32 (exact), the op runs in fp32 and
the result is rounded once; integers wrap (computed on numpy's unsigned views, where wrapping is
defined); MAX is `a if isnan(a) else (b if isnan(b) else (a if a > b else b))` with a = target,
MIN alike; LAND / LOR / LXOR give 0 / 1 in the dtype.

Every comparison is bitwise and over whole buffers: the target sits between 64 sentinel bytes on
each side and starts as sentinels in the gaps between its runs, the fetch stream sits between
sentinels, and the origin stream must come back unchanged.

Float data holds +-inf, NaN, denormals and pairs whose sum needs the single rounding (1 + eps/2 *
(1 + eps) rounds up from fp32, while a sum of operands rounded to the result's ulp first would
tie to even). It holds no pair that makes an invalid operation (inf - inf, 0 * inf) and no pair
of NaNs: the payload of a NaN made or chosen there is the processor's, not IEEE's, and the host
oracle could not name the device's bits. A NaN operand is the canonical quiet NaN, which every
processor passes through. MAX / MIN never see +0.0 against -0.0.

The CPU tier runs the host twin, the gpu tier the kernel on the same cases."""
import numpy as np
import pytest
import torch

from mpit_amd import datatypes as dt
from mpit_amd._ext import native

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
G, SENT = 64, 0xA5
OPS = ["SUM", "PROD", "MAX", "MIN", "LAND", "LOR", "LXOR", "BAND", "BOR", "BXOR", "REPLACE", "NO_OP"]  # = the codes
# name -> (torch dtype, PeerDtype code, basic MPI type)
TYPES = {"f32": (torch.float32, 0, dt.FLOAT), "bf16": (torch.bfloat16, 1, dt.BFLOAT16), "f16": (torch.float16, 2, dt.HALF),
         "f64": (torch.float64, 3, dt.DOUBLE), "i32": (torch.int32, 4, dt.INT), "i64": (torch.int64, 5, dt.LONG),
         "u8": (torch.uint8, 6, dt.BYTE)}
_UNSIGNED = {torch.int32: np.uint32, torch.int64: np.uint64, torch.uint8: np.uint8}


def supported(op, tdt):
    return not (op in ("BAND", "BOR", "BXOR") and tdt.is_floating_point)


def type_index(t, count):
    """Byte index of every packed byte, from the type map's definition."""
    idx = []
    for i in range(count):
        for d, b in t.typemap:
            idx.extend(range(i * t.extent + d, i * t.extent + d + dt._BASIC[b][0]))
    return np.array(idx, dtype=np.int64)


def indexed_type(R, equal, seed, step=1):
    """R runs at seeded, sorted, non-overlapping, non-adjacent byte offsets (multiples of step)."""
    rng = np.random.default_rng(seed)
    lens = np.full(R, 8 * step) if equal else rng.integers(1, 17, R) * step
    gaps = rng.integers(1, 9, R) * step
    offs = np.concatenate([[0], np.cumsum(lens + gaps)[:-1]])
    return dt.Type_create_hindexed([int(x) for x in lens], [int(x) for x in offs], dt.BYTE)


def make_data(tdt, n, seed):
    """(target, origin) host tensors of n elements; see the module docstring for what they hold."""
    rng = np.random.default_rng(seed)
    if tdt.is_floating_point:
        t = torch.from_numpy(rng.integers(-64, 65, n) / 8.0).to(tdt)
        o = torch.from_numpy(rng.integers(-64, 65, n) / 8.0).to(tdt)
        fi = torch.finfo(tdt)
        inf, nan, tiny, eps = float("inf"), float("nan"), fi.tiny, fi.eps
        pairs = [(inf, 1.5), (2.5, -inf), (nan, 3.0), (-2.0, nan), (tiny / 4, tiny / 2), (tiny / 4, 3 * tiny / 4),
                 (1.0, eps / 2 * (1 + eps)), (1.0, eps / 2), (-inf, -inf), (-tiny / 2, tiny / 4)]
        for k, (a, b) in enumerate(pairs[:n]):
            t[k] = torch.tensor(a, dtype=torch.float64).to(tdt)
            o[k] = torch.tensor(b, dtype=torch.float64).to(tdt)
        return t, o
    if tdt == torch.uint8:
        t, o = (torch.from_numpy(rng.integers(0, 256, n, dtype=np.uint8)) for _ in range(2))
    else:
        ii = torch.iinfo(tdt)
        t, o = (torch.from_numpy(rng.integers(ii.min, ii.max, n, dtype=np.int64, endpoint=True)).to(tdt) for _ in range(2))
    t[::5] = 0  # the logical ops need zeros on either side, and on both
    o[::3] = 0
    return t, o


def narrow(r, tdt):
    """Round to nearest even, once. A NaN keeps its sign and its quiet bit and drops the low payload
    bits, as the hardware conversions and the host's do (torch's own cast sets every payload bit)."""
    out = r.to(tdt)
    if tdt in (torch.bfloat16, torch.float16):
        bits = r.contiguous().view(torch.int32)
        if tdt == torch.bfloat16:
            nan = (bits >> 16) | 0x0040
        else:
            nan = ((bits >> 16) & 0x8000) | 0x7E00 | ((bits >> 13) & 0x01FF)
        out = torch.where(torch.isnan(r), nan.to(torch.int16).view(tdt), out)
    return out


def oracle(op, t, o):
    """comb(op, target, origin) per element, on the host."""
    if op == "REPLACE":
        return o.clone()
    if op == "NO_OP":
        return t.clone()
    tdt = t.dtype
    if tdt.is_floating_point:
        a, b = (t.float(), o.float()) if tdt in (torch.bfloat16, torch.float16) else (t, o)
        if op == "SUM":
            r = a + b
        elif op == "PROD":
            r = a * b
        elif op == "MAX":
            r = torch.where(torch.isnan(a), a, torch.where(torch.isnan(b), b, torch.where(a > b, a, b)))
        elif op == "MIN":
            r = torch.where(torch.isnan(a), a, torch.where(torch.isnan(b), b, torch.where(a < b, a, b)))
        else:
            ta, tb = a != 0, b != 0
            r = {"LAND": ta & tb, "LOR": ta | tb, "LXOR": ta ^ tb}[op].to(a.dtype)
        return narrow(r, tdt)  # the one rounding
    a, b = t.numpy(), o.numpy()
    ua, ub = a.view(_UNSIGNED[tdt]), b.view(_UNSIGNED[tdt])
    if op == "SUM":
        r = (ua + ub).view(a.dtype)
    elif op == "PROD":
        r = (ua * ub).view(a.dtype)
    elif op == "MAX":
        r = np.where(a > b, a, b)
    elif op == "MIN":
        r = np.where(a < b, a, b)
    elif op in ("LAND", "LOR", "LXOR"):
        ta, tb = a != 0, b != 0
        r = {"LAND": ta & tb, "LOR": ta | tb, "LXOR": ta ^ tb}[op].astype(a.dtype)
    else:
        r = {"BAND": ua & ub, "BOR": ua | ub, "BXOR": ua ^ ub}[op].view(a.dtype)
    return torch.from_numpy(np.ascontiguousarray(r))


def as_bytes(x):
    return x.contiguous().view(torch.uint8).numpy()


def dev_of(device):
    if device == "cpu":
        return -1, 0
    return torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream


def check(device, tname, op, t, count, fetch=False, soff=0, poff=0, foff=0, max_blocks=0, wide=False, seed=0,
          unit=None, no_origin=False, raises=None):
    """One type_accumulate call of `count` x t (a layout of whole `tname` elements) with the target
    base `soff`, the origin stream `poff` and the fetch stream `foff` bytes into 16-byte-aligned
    allocations; the whole target, origin and fetch buffers against the oracle. With `raises` the
    call must raise that and leave every buffer as it was. Returns (plan, the target's bytes)."""
    tdt, dcode, _ = TYPES[tname]
    es = torch.empty(0, dtype=tdt).element_size()
    idx = type_index(t, count)
    ne = len(idx) // es
    starts = idx.reshape(ne, es)
    assert (np.diff(starts, axis=1) == 1).all()  # the layout holds whole elements
    tv, ov = make_data(tdt, ne, seed)
    nb = int(idx.max()) + 1
    tbuf = np.full(G + soff + nb + G, SENT, dtype=np.uint8)
    tbuf[G + soff + idx] = as_bytes(tv)
    obuf = np.full(G + poff + ne * es + G, SENT, dtype=np.uint8)
    obuf[G + poff: G + poff + ne * es] = as_bytes(ov)
    fbuf = np.full(G + foff + ne * es + G, SENT, dtype=np.uint8)
    T, O, F = (torch.from_numpy(x.copy()).to(device) for x in (tbuf, obuf, fbuf))
    assert T.data_ptr() % 16 == 0 and O.data_ptr() % 16 == 0 and F.data_ptr() % 16 == 0
    plan = t.plan(count)
    tab, off, _keep = plan.table(T.device)
    sp = T.data_ptr() + G + soff + off
    pp = 0 if no_origin else O.data_ptr() + G + poff
    fp = F.data_ptr() + G + foff if fetch else 0
    u = plan.unit(sp, pp | fp)
    if unit is not None:
        assert u == unit, (plan, soff, poff, foff, u)
    dev, stream = dev_of(device)
    args = (dev, stream, OPS.index(op), dcode, sp, pp, fp, plan._loops, tab, plan.R, plan.L, plan.per, u, max_blocks, wide)
    if raises is not None:
        with pytest.raises(raises):
            native().type_accumulate(*args)
        want_t, want_f = tbuf, fbuf
    else:
        native().type_accumulate(*args)
        want_t = tbuf.copy()
        want_t[G + soff + idx] = as_bytes(oracle(op, tv, ov))
        want_f = fbuf.copy()
        if fetch:
            want_f[G + foff: G + foff + ne * es] = as_bytes(tv)
    got_t, got_o, got_f = T.cpu().numpy(), O.cpu().numpy(), F.cpu().numpy()
    where = (tname, op, t, count, soff, poff, foff, max_blocks, wide)
    assert np.array_equal(got_t, want_t), (where, np.flatnonzero(got_t != want_t)[:8])
    assert np.array_equal(got_o, obuf), where
    assert np.array_equal(got_f, want_f), (where, np.flatnonzero(got_f != want_f)[:8])
    return plan, got_t


# ------------------------------------------------------------------ the op x type table
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("tname", list(TYPES))
def test_every_op_on_every_type(device, tname):
    tdt, dcode, basic = TYPES[tname]
    vec = dt.Type_vector(5, 3, 7, basic)
    for k, op in enumerate(OPS):
        if supported(op, tdt):
            assert native().type_accumulate_supported(OPS.index(op), dcode)
            check(device, tname, op, vec, 2, fetch=bool(k & 1), seed=k)
        else:  # refused before any launch: nothing moves
            assert not native().type_accumulate_supported(OPS.index(op), dcode)
            check(device, tname, op, vec, 2, fetch=True, seed=k, raises=ValueError)


def test_the_oracle_sees_the_single_rounding():
    """The data does hold a pair whose bf16 / fp16 sum tells one rounding from two."""
    for tdt in (torch.bfloat16, torch.float16):
        t, o = make_data(tdt, 30, 0)
        eps = torch.finfo(tdt).eps
        s = oracle("SUM", t, o)
        assert float(s[6]) == 1.0 + eps and float(s[7]) == 1.0  # just above the tie: up; the tie: to even
        assert float(t[6]) + float(o[6]) not in (1.0, 1.0 + eps) and float(o[6]) - eps / 2 < eps / 2  # inexact, and
        # an origin rounded to the sum's precision before the addition (eps / 2, a tie) would give 1.0 instead
        assert bool(torch.isnan(oracle("MAX", t, o)[2])) and bool(torch.isnan(oracle("MIN", t, o)[3]))
        assert 0 < float(t[4]) < torch.finfo(tdt).tiny  # a denormal


# ------------------------------------------------------------------ run modes
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("R,equal", [(1, True), (2, True), (2, False), (3, True), (3, False), (65, True), (65, False),
                                     (1024, True), (1024, False), (1025, True), (1025, False)])
def test_run_tables(device, R, equal):
    """R == 1 needs no table; equal lengths map by division, unequal ones by binary search of the
    prefix sums; R <= 1024 stages the table in LDS, 1025 reads it from global memory."""
    for tname, step, op in (("f32", 4, "SUM"), ("u8", 1, "BXOR"), ("i64", 8, "MIN")):
        t = indexed_type(R, equal, seed=100 + R, step=step)
        plan, _ = check(device, tname, op, t, 2, fetch=True, seed=R)
        assert plan.align >= step
        if R >= 65:
            assert plan.R == R and plan.L == (8 * step if equal else 0)
        if R == 1:
            assert plan.table(torch.device("cpu"))[0] == 0


# ------------------------------------------------------------------ unit selection
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("tname", ["u8", "bf16", "f16", "i32", "f32", "f64", "i64"])
def test_unit_selection(device, tname):
    """Every item size from 16 bytes down to the element's own, made by the base addresses and by
    the layout; a base that would make an item smaller than an element is refused."""
    tdt = TYPES[tname][0]
    es = torch.empty(0, dtype=tdt).element_size()
    wide16 = dt.Type_create_hvector(5, 48, 80, dt.BYTE)  # the layout allows 16
    units = [u for u in (16, 8, 4, 2, 1) if u >= es]
    for u in units:
        for which in range(3):  # the target, the origin, the fetch stream lowers the unit
            offs = [0, 0, 0]
            offs[which] = u % 16
            check(device, tname, "SUM", wide16, 1, fetch=True, soff=offs[0], poff=offs[1], foff=offs[2], seed=u, unit=u)
        if u < 16:  # and the layout itself: runs of 3 items
            t = dt.Type_create_hvector(5, 3 * u, 5 * u, dt.BYTE)
            if (3 * u) % es == 0:
                check(device, tname, "MAX", t, 2, fetch=False, seed=u + 1, unit=u)
    if es > 1:
        for which in range(3):
            offs = [0, 0, 0]
            offs[which] = es // 2
            check(device, tname, "SUM", wide16, 1, fetch=True, soff=offs[0], poff=offs[1], foff=offs[2], unit=es // 2,
                  raises=ValueError)


# ------------------------------------------------------------------ seams and grid-stride
@pytest.mark.parametrize("device", DEVICES)
def test_tile_seams(device):
    """1,024 items per block and round: one short, exact, one over, and the same around two."""
    for items in (1023, 1024, 1025, 2047, 2048, 2049):
        check(device, "f32", "SUM", dt.Type_create_hvector(items, 16, 48, dt.BYTE), 1, fetch=True, seed=items, unit=16)
        check(device, "f32", "PROD", dt.Type_create_hvector(items, 4, 12, dt.BYTE), 1, seed=items + 1, unit=4)
        check(device, "bf16", "SUM", dt.Type_create_hvector(items, 2, 6, dt.BYTE), 1, fetch=True, seed=items + 2, unit=2)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("wide", [False, True])
def test_grid_stride_and_index_width(device, wide):
    """max_blocks 1 and 2 over 5 tiles (4,613 items), without and with a run table, both index
    widths: the same bytes as the default launch (and as the oracle)."""
    t1 = dt.Type_create_hvector(4613, 4, 12, dt.BYTE)  # unit 4, no table
    t2 = dt.Type_create_hindexed([12, 4, 24], [4, 24, 36], dt.BYTE)  # irregular: the table path
    for t, count in ((t1, 1), (t2, 461)):
        ref = check(device, "i32", "SUM", t, count, fetch=True, seed=7, unit=4)[1]
        for mb in (1, 2):
            plan, got = check(device, "i32", "SUM", t, count, fetch=True, seed=7, unit=4, max_blocks=mb, wide=wide)
            assert 4 * 1024 < plan.total // 4 <= 5 * 1024 and np.array_equal(got, ref)


# ------------------------------------------------------------------ fetch
@pytest.mark.parametrize("device", DEVICES)
def test_fetch_forms(device):
    vec = dt.Type_vector(5, 3, 7, dt.FLOAT)
    irr = dt.Type_create_hindexed([12, 4, 24], [4, 24, 36], dt.BYTE)
    for t, count in ((vec, 2), (irr, 3)):
        check(device, "f32", "SUM", t, count, fetch=True, seed=1)  # fetch and op
        check(device, "f32", "NO_OP", t, count, fetch=True, seed=2)  # an atomic get: the target keeps its bits
        check(device, "f32", "NO_OP", t, count, fetch=True, seed=2, no_origin=True)  # ... without an origin at all
        check(device, "f32", "REPLACE", t, count, fetch=True, seed=3)  # a swap
        check(device, "f32", "NO_OP", t, count, fetch=False, seed=4)  # nothing to do
    check(device, "f32", "SUM", vec, 2, seed=5, no_origin=True, raises=ValueError)


# ------------------------------------------------------------------ loops
@pytest.mark.parametrize("device", DEVICES)
def test_loops(device):
    sub = dt.Type_create_subarray([6, 5, 8], [3, 2, 4], [2, 1, 3], dt.ORDER_C, dt.FLOAT)
    plan, _ = check(device, "f32", "MAX", sub, 2, fetch=True, seed=1)
    assert len(plan.loops) == 3 and plan.R == 1
    pad = dt.Type_create_resized(dt.Type_vector(3, 1, 2, dt.INT), 0, 24)  # instances continue the type's own loop
    plan, _ = check(device, "i32", "PROD", pad, 4, fetch=True, seed=2)
    assert plan.loops == ((12, 8),)
    s = dt.Type_create_struct([1, 2], [0, 8], [dt.INT, dt.INT])  # a table under a count loop
    plan, _ = check(device, "i32", "BOR", s, 3, seed=3)
    assert plan.R == 2 and plan.loops == ((3, 16),)
    for tname, basic in (("f64", dt.DOUBLE), ("f16", dt.HALF)):
        check(device, tname, "SUM", dt.Type_contiguous(37, basic), 3, fetch=True, seed=4)  # one contiguous run


# ------------------------------------------------------------------ bad arguments
def test_raw_binding_refuses_inconsistent_arguments():
    nat = native()
    x, y, z = (torch.zeros(64, dtype=torch.uint8) for _ in range(3))
    ok = dict(dev=-1, stream=0, op=0, dtype=0, strided=x.data_ptr(), packed=y.data_ptr(), fetch=z.data_ptr(),
              loops=[(2, 16)], table=0, R=1, L=8, per=8, unit=8)
    y[:] = 1
    nat.type_accumulate(**ok)
    assert int(x.view(torch.int32).ne(0).sum()) == 4  # four float sums changed, the rest untouched
    before = x.clone()
    for bad in (dict(unit=3), dict(unit=32), dict(R=2), dict(per=12), dict(L=0), dict(loops=[(2, 4)]),
                dict(strided=x.data_ptr() + 4), dict(packed=y.data_ptr() + 2), dict(fetch=z.data_ptr() + 4),
                dict(loops=[(1, 1)] * 4), dict(loops=[(-1, 16)]), dict(op=12), dict(op=-1), dict(dtype=7), dict(dtype=-1),
                dict(op=7), dict(dtype=3, unit=4, L=4, per=4), dict(strided=0), dict(packed=0)):
        with pytest.raises(ValueError):
            nat.type_accumulate(**{**ok, **bad})
    assert torch.equal(x, before) and not z[16:].any()


# ------------------------------------------------------------------ the all-reduce's bits
@pytest.mark.parametrize("device", DEVICES)
def test_same_bits_as_the_all_reduce(device):
    """type_accumulate of b onto a == peer_reduce over [a, b], bitwise: they share comb."""
    nat = native()
    dev, stream = dev_of(device)
    n = 1031
    for tname, op in (("f32", "SUM"), ("f32", "PROD"), ("bf16", "SUM"), ("bf16", "PROD"), ("i32", "BXOR")):
        tdt, dcode, _ = TYPES[tname]
        es = torch.empty(0, dtype=tdt).element_size()
        a, b = (x.to(device) for x in make_data(tdt, n, 40 + dcode))
        out = torch.zeros(n, dtype=tdt, device=device)
        nat.peer_reduce(dev, stream, OPS.index(op), dcode, [a.data_ptr(), b.data_ptr()], [out.data_ptr()], n)
        acc = a.clone()
        nat.type_accumulate(dev, stream, OPS.index(op), dcode, acc.data_ptr(), b.data_ptr(), 0, [], 0, 1, n * es, n * es, es)
        assert np.array_equal(as_bytes(acc.cpu()), as_bytes(out.cpu())), (tname, op)
        assert np.array_equal(as_bytes(out.cpu()), as_bytes(oracle(op, a.cpu(), b.cpu()))), (tname, op)
