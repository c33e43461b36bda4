"""Derived datatypes in one launch: the layout plan (mpit_amd/datatypes.py Plan / layout_of), the
type_copy kernel and its host twin (csrc/kernels/type_copy.hip) and the routing of pack / unpack /
Pack / Unpack / Pack_external through them.

The oracle is the type map's definition, byte by byte, in numpy: instance i of a type places the
bytes of entry (d, basic) at i * extent + d ... + size. It never calls Datatype.pack or
_byte_index. Every comparison is bitwise and over whole buffers: packed outputs sit between 64
sentinel bytes on each side, unpack targets start as sentinels, so a stray store anywhere fails.
The CPU tier runs the host twin, the gpu tier the kernel on the same cases."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mpit_amd import datatypes as dt
from mpit_amd._ext import native

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
G, SENT = 64, 0xA5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def type_index(t, count):
    """Byte index of every packed byte, from the type map's definition."""
    idx = []
    for i in range(count):
        for d, b in t.typemap:
            idx.extend(range(i * t.extent + d, i * t.extent + d + dt._BASIC[b][0]))
    return np.array(idx, dtype=np.int64)


def low_bit(x):
    return 16 if x % 16 == 0 else (x & -x)


def rand_bytes(n, seed):
    return np.random.default_rng(seed).integers(1, 256, n, dtype=np.uint8)  # never 0, never a sentinel run


def dev_bytes(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def check_type(t, count, device, unpack=True, soff=0, poff=0, seed=0, unit=None):
    """pack and (optionally) unpack `count` x t with the strided view `soff` bytes and the packed
    view `poff` bytes into 16-byte-aligned allocations; whole buffers against the oracle."""
    idx = type_index(t, count)
    n = len(idx)
    nb = (int(idx.max()) + 1 if n else 0) + 5
    host = rand_bytes(soff + nb, seed)
    src = dev_bytes(host, device)
    outbuf = torch.full((G + poff + n + G,), SENT, dtype=torch.uint8, device=device)
    assert src.data_ptr() % 16 == 0 and outbuf.data_ptr() % 16 == 0
    out = outbuf[G + poff: G + poff + n]
    before = dict(dt.COUNTERS)
    got = t.pack(src[soff:], count, out=out)
    assert got.data_ptr() == out.data_ptr()
    exp = np.full(G + poff + n + G, SENT, dtype=np.uint8)
    exp[G + poff: G + poff + n] = host[soff:][idx]
    assert np.array_equal(outbuf.cpu().numpy(), exp), (t, count, soff, poff)
    plan = t.plan(count)
    if unit is not None:
        assert plan.unit(src.data_ptr() + soff, out.data_ptr()) == unit, (plan, soff, poff)
    if n:
        assert dt.COUNTERS["kernel"] == before["kernel"] + 1 and dt.COUNTERS["index"] == before["index"]
    if unpack:
        tgt = torch.full((soff + nb,), SENT, dtype=torch.uint8, device=device)
        t.unpack(out, tgt[soff:], count)
        exp = np.full(soff + nb, SENT, dtype=np.uint8)
        exp[soff:][idx] = host[soff:][idx]
        assert np.array_equal(tgt.cpu().numpy(), exp), (t, count, soff, poff)
    return plan


def indexed_type(R, equal, seed, step=1):
    """R runs at seeded, sorted, non-overlapping, non-adjacent byte offsets (multiples of step)."""
    rng = np.random.default_rng(seed)
    lens = np.full(R, 8 * step) if equal else rng.integers(1, 17, R) * step
    gaps = rng.integers(1, 9, R) * step
    offs = np.concatenate([[0], np.cumsum(lens + gaps)[:-1]])
    return dt.Type_create_hindexed([int(x) for x in lens], [int(x) for x in offs], dt.BYTE), lens


# ------------------------------------------------------------------ unit selection
@pytest.mark.parametrize("device", DEVICES)
def test_unit_selection_and_bytes(device):
    for b, s in [(1, 3), (2, 6), (4, 12), (8, 24), (16, 48), (48, 80), (12, 20)]:
        t = dt.Type_create_hvector(5, b, s, dt.BYTE)
        for soff in (0, 1, 2, 4, 8):
            for poff in (0, 1, 4):
                unit = min(low_bit(b), low_bit(s), low_bit(soff), low_bit(poff))
                plan = check_type(t, 1, device, soff=soff, poff=poff, seed=b + soff, unit=unit)
                assert plan.R == 1 and plan.L == b and plan.loops == ((5, s),)
    assert dt.Type_create_hvector(5, 48, 80, dt.BYTE).plan(1).align == 16
    assert dt.Type_create_hvector(5, 12, 20, dt.BYTE).plan(1).align == 4


# ------------------------------------------------------------------ table and uniform paths
@pytest.mark.parametrize("device", DEVICES)
def test_indexed_small_tables(device):
    a = dt.Type_create_hindexed([4, 8, 4], [0, 8, 24], dt.BYTE)
    b = dt.Type_create_hindexed([16, 1, 16, 3], [0, 20, 32, 64], dt.BYTE)
    pa, pb = check_type(a, 2, device, seed=1), check_type(b, 3, device, seed=2)
    assert (pa.R, pa.L, pa.align) == (3, 0, 4) and (pb.R, pb.L, pb.align) == (4, 0, 1)
    assert pa.prefix.tolist() == [0, 4, 12, 16] and pb.offs.tolist() == [0, 20, 32, 64]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("R,equal", [(1, True), (1, False), (2, True), (2, False), (3, True), (3, False), (65, True),
                                     (65, False), (1025, True), (1025, False)])
def test_run_tables(device, R, equal):
    """R <= 1024 stages the table in LDS, 1025 reads it from global memory; equal lengths map by
    division, unequal ones by binary search of the prefix sums. An irregular table stays whole."""
    for step in (1, 4):
        t, lens = indexed_type(R, equal, seed=100 + R, step=step)
        plan = check_type(t, 2, device, seed=R)
        assert plan.align >= step
        if R >= 65:  # (two or three seeded runs may happen to be a progression and fold)
            assert plan.R == R and plan.loops == ((2, t.extent),)
            assert plan.L == (8 * step if equal else 0) and (len(set(lens.tolist())) == 1) == equal
        else:
            assert plan.R <= R and (plan.L != 0) == (plan.R == 1 or len(set(plan.lens.tolist())) == 1)


# ------------------------------------------------------------------ folding
@pytest.mark.parametrize("device", DEVICES)
def test_folding(device):
    v = dt.Type_vector(4096, 4, 8, dt.FLOAT)
    p = check_type(v, 1, device, seed=3)
    assert p.R == 1 and p.L == 16 and p.loops == ((4096, 32),) and p.align == 16
    assert check_type(v, 2, device, seed=4).loops == ((2, v.extent), (4096, 32))
    for order in (dt.ORDER_C, dt.ORDER_FORTRAN):
        sub = dt.Type_create_subarray([6, 5, 8], [3, 2, 4], [2, 1, 3], order, dt.FLOAT)
        p = check_type(sub, 2, device, seed=5 + order)
        outer = 3 * 2 if order == dt.ORDER_C else 4 * 2
        assert p.R <= outer and len(p.loops) <= 3
        assert p.R == 1 and p.loops[0] == (2, 6 * 5 * 8 * 4)  # folds all the way
    sub2 = dt.Type_create_subarray([7, 9], [3, 4], [2, 5], dt.ORDER_C, dt.DOUBLE)
    assert check_type(sub2, 3, device, seed=8).R == 1
    s = dt.Type_create_struct([1, 2], [0, 8], [dt.INT, dt.FLOAT]).Commit()  # tests/test_units.py:53
    p = check_type(s, 3, device, seed=6)
    assert p.R == 2 and p.L == 0 and p.loops == ((3, 16),) and p.align == 4
    rz = dt.Type_create_resized(dt.Type_vector(2, 1, 2, dt.INT), 0, 4)  # instances interleave: pack only
    p = check_type(rz, 3, device, unpack=False, seed=7)
    assert p.R == 1 and p.loops == ((3, 4), (2, 8))
    # contiguous instances become one run; instances that continue the type's own loop extend it
    assert dt.Type_contiguous(5, dt.FLOAT).plan(7).loops == () and check_type(dt.Type_contiguous(5, dt.FLOAT), 7, device).L == 140
    pad = dt.Type_create_resized(dt.Type_vector(3, 1, 2, dt.INT), 0, 24)
    assert check_type(pad, 4, device, seed=9).loops == ((12, 8),)


def test_plan_cost_is_per_type_not_per_count():
    v = dt.Type_vector(4096, 4, 8, dt.FLOAT)
    p1, p2 = v.plan(1), v.plan(1 << 20)
    assert v.plan(1) is p1 and p2.R == 1 and p2.total == (1 << 20) * 65536 and p2.offs is p1.offs
    t, _ = indexed_type(65, False, seed=1)
    assert t.plan(3)._tables is t.plan(5)._tables  # one uploaded table per (type, device)
    tab1 = t.plan(3).table(torch.device("cpu"))[2]
    assert t.plan(5).table(torch.device("cpu"))[2] is tab1 and tab1.dtype == torch.int64 and tab1.numel() == 2 * 65 + 1


# ------------------------------------------------------------------ seams and grid-stride
@pytest.mark.parametrize("device", DEVICES)
def test_tile_seams(device):
    for b, s in [(1, 3), (4, 12), (16, 48)]:
        for k in (1, 2):
            for d in (-16, 0, 16):
                n = (k * 4096 + d) // b
                check_type(dt.Type_create_hvector(n, b, s, dt.BYTE), 1, device, seed=100 * k + 16 + d, unit=low_bit(b))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("wide", [False, True])
def test_raw_binding_grid_stride(device, wide):
    """max_blocks 1 and 2 on a stream of 10,540 one-byte items (1,024 per block and round: 11 and 6
    rounds), with and without a table, both directions, both index widths."""
    nat = native()
    dev = -1 if device == "cpu" else torch.cuda.current_device()
    stream = 0 if device == "cpu" else torch.cuda.current_stream().cuda_stream
    t1 = dt.Type_create_hvector(2108, 5, 7, dt.BYTE)  # 10,540 bytes, unit 1, no table
    t2 = dt.Type_create_hindexed([3, 1, 6], [1, 6, 9], dt.BYTE)  # irregular: the table path, count 1054
    for t, count in ((t1, 1), (t2, 1054)):
        plan = t.plan(count)
        assert plan.total == 10540 and plan.align == 1
        idx = type_index(t, count)
        nb = int(idx.max()) + 1 + 5
        host = rand_bytes(nb, 11)
        src = dev_bytes(host, device)
        tab, off, keep = plan.table(src.device)
        assert (tab == 0) == (plan.R == 1)
        for mb in (1, 2):
            outbuf = torch.full((G + plan.total + G,), SENT, dtype=torch.uint8, device=device)
            out = outbuf[G: G + plan.total]
            nat.type_copy(dev, stream, 0, src.data_ptr() + off, out.data_ptr(), list(plan.loops), tab, plan.R, plan.L,
                          plan.per, 1, mb, wide)
            exp = np.full(G + plan.total + G, SENT, dtype=np.uint8)
            exp[G: G + plan.total] = host[idx]
            assert np.array_equal(outbuf.cpu().numpy(), exp), (t, mb)
            tgt = torch.full((nb,), SENT, dtype=torch.uint8, device=device)
            nat.type_copy(dev, stream, 1, tgt.data_ptr() + off, out.data_ptr(), list(plan.loops), tab, plan.R, plan.L,
                          plan.per, 1, mb, wide)
            exp = np.full(nb, SENT, dtype=np.uint8)
            exp[idx] = host[idx]
            assert np.array_equal(tgt.cpu().numpy(), exp), (t, mb)


def test_raw_binding_refuses_inconsistent_arguments():
    nat = native()
    x, y = torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    ok = dict(dev=-1, stream=0, dir=0, strided=x.data_ptr(), packed=y.data_ptr(), loops=[(2, 16)], table=0, R=1, L=8,
              per=8, unit=8)
    nat.type_copy(**ok)
    for bad in (dict(unit=3), dict(unit=32), dict(dir=2), dict(R=2), dict(per=12), dict(L=0), dict(loops=[(2, 4)]),
                dict(strided=x.data_ptr() + 4), dict(packed=y.data_ptr() + 2), dict(loops=[(1, 1)] * 4),
                dict(loops=[(-1, 16)])):
        with pytest.raises(Exception):
            nat.type_copy(**{**ok, **bad})


# ------------------------------------------------------------------ counts
@pytest.mark.parametrize("device", DEVICES)
def test_counts_and_empty_type(device):
    t = dt.Type_create_hindexed([4, 8, 4], [0, 8, 24], dt.BYTE)
    for count in (0, 1, 2, 7):
        check_type(t, count, device, seed=count)
    before = dict(dt.COUNTERS)
    for empty, count in ((dt.Type_contiguous(0, dt.FLOAT), 3), (dt.Type_create_struct([], [], []), 2), (t, 0)):
        src = torch.arange(64, dtype=torch.uint8, device=device)
        got = empty.pack(src, count)
        assert got.numel() == 0 and got.dtype == torch.uint8 and got.device == src.device
        empty.unpack(got, src, count)
        assert src.cpu().tolist() == list(range(64))
    assert dt.COUNTERS == before  # no launch, no index op


# ------------------------------------------------------------------ 64-bit offsets (GPU only)
@pytest.mark.gpu
def test_offsets_beyond_2_31():
    ext = (1 << 31) + 16
    t = dt.Type_create_resized(dt.Type_contiguous(16, dt.BYTE), 0, ext)
    nb = (1 << 31) + 96
    buf = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    data = dev_bytes(rand_bytes(32, 5), "cuda")
    buf[:16] = data[:16]
    buf[ext: ext + 16] = data[16:]
    plan = t.plan(2)
    assert plan.loops == ((2, ext),) and plan.hi == ext + 16 and plan.total == 32
    outbuf = torch.full((G + 32 + G,), SENT, dtype=torch.uint8, device="cuda")
    t.pack(buf, 2, out=outbuf[G: G + 32])
    exp = torch.full((G + 32 + G,), SENT, dtype=torch.uint8)
    exp[G: G + 32] = data.cpu()
    assert torch.equal(outbuf.cpu(), exp)
    buf.zero_()
    t.unpack(outbuf[G: G + 32], buf, 2)
    assert torch.equal(buf[:16], data[:16]) and torch.equal(buf[ext: ext + 16], data[16:])
    assert int(torch.count_nonzero(buf)) == 32  # the data bytes are never 0: nothing else was written
    with pytest.raises(IndexError):
        t.pack(buf[: nb - 96 + 15], 2)


# ------------------------------------------------------------------ front ends
@pytest.mark.parametrize("device", DEVICES)
def test_pack_unpack_positions_and_external(device):
    vec = dt.Type_vector(3, 2, 4, dt.INT)
    idx = type_index(vec, 2)
    host = rand_bytes(int(idx.max()) + 1, 21)
    src = dev_bytes(host, device)
    out = torch.full((100,), SENT, dtype=torch.uint8, device=device)
    before = dt.COUNTERS["kernel"]
    pos = dt.Pack(src, 2, vec, out, 7)
    assert pos == 7 + 48 and dt.COUNTERS["kernel"] == before + 1
    exp = np.full(100, SENT, dtype=np.uint8)
    exp[7:55] = host[idx]
    assert np.array_equal(out.cpu().numpy(), exp)
    tgt = torch.full((len(host),), SENT, dtype=torch.uint8, device=device)
    assert dt.Unpack(out, 7, tgt, 2, vec) == 55
    exp = np.full(len(host), SENT, dtype=np.uint8)
    exp[idx] = host[idx]
    assert np.array_equal(tgt.cpu().numpy(), exp)
    # external32: every basic element big-endian in the stream, restored by the round trip
    a = torch.arange(1, 21, dtype=torch.int32, device=device) * 0x01020304
    ext = torch.full((64,), SENT, dtype=torch.uint8, device=device)
    end = dt.Pack_external("external32", a, 2, vec, ext, 5)
    assert end == 5 + 48
    exp = np.full(64, SENT, dtype=np.uint8)
    exp[5:53] = a.cpu().numpy().view(np.uint8)[idx].reshape(-1, 4)[:, ::-1].reshape(-1)
    assert np.array_equal(ext.cpu().numpy(), exp)
    back = torch.zeros(20, dtype=torch.int32, device=device)
    assert dt.Unpack_external("external32", ext, 5, back, 2, vec) == 53
    want = np.zeros(80, dtype=np.uint8)
    want[idx] = a.cpu().numpy().view(np.uint8)[idx]
    assert np.array_equal(back.cpu().numpy().view(np.uint8), want)


def strided_views(device):
    x = torch.arange(6 * 10, dtype=torch.float32, device=device).reshape(6, 10)
    y = torch.arange(2 * 3 * 4 * 5, dtype=torch.int16, device=device).reshape(2, 3, 4, 5)
    return {"cols": x[:, 1:5], "t": x.t(), "channels_last": y.contiguous(memory_format=torch.channels_last),
            "step": x[::3], "rows_step": x.reshape(-1)[::3], "expand": x[0:1, :].expand(4, 10)}


@pytest.mark.parametrize("device", DEVICES)
def test_layout_of_strided_tensors(device):
    views = strided_views(device)
    loops = {"cols": ((6, 40),), "t": ((10, 4), (6, 40)), "channels_last": ((2, 120), (3, 2), (20, 6)),
             "step": ((2, 120),), "rows_step": ((20, 12),), "expand": ((4, 0),)}
    runs = {"cols": 16, "t": 4, "channels_last": 2, "step": 40, "rows_step": 4, "expand": 40}
    for name, v in views.items():
        assert not v.is_contiguous() or name == "expand"
        plan = dt.layout_of(v)
        assert plan.loops == loops[name] and plan.R == 1 and plan.L == runs[name], (name, plan)
        # the oracle: element (i, j, ...) in row-major order lives at sum(i_k * stride_k) elements
        es = v.element_size()
        grid = np.indices(v.shape).reshape(v.dim(), -1)
        elem = (grid * np.array(v.stride()).reshape(-1, 1)).sum(0)
        base = torch.as_strided(v, (int(elem.max()) + 1,), (1,)).cpu().numpy()
        before = dt.COUNTERS["kernel"]
        got = dt.pack_tensor(v)
        assert dt.COUNTERS["kernel"] == before + 1
        assert got.dtype == v.dtype and np.array_equal(got.cpu().numpy().view(np.uint8), base[elem].view(np.uint8))
        if name == "expand":
            with pytest.raises(ValueError):
                dt.unpack_tensor(got, v)
            continue
        # scatter back into a sentinel-filled storage of the same geometry: only the view's bytes change
        store = torch.full((int(elem.max()) + 1 + 3,), -3, dtype=v.dtype, device=device)
        tgt = torch.as_strided(store, v.shape, v.stride())
        dt.unpack_tensor(got, tgt)
        want = np.full(store.numel(), -3, dtype=base.dtype)
        want[elem] = base[elem]
        assert np.array_equal(store.cpu().numpy().view(np.uint8), want.view(np.uint8)), name
    overlapping = torch.as_strided(torch.zeros(16, device=device), (3, 4), (2, 1))
    with pytest.raises(ValueError):
        dt.check_writable_layout(overlapping)
    five = torch.zeros(2, 4, 2, 4, 2, 4, 2, 4, 2, 2, device=device)[:, ::2, :, ::2, :, ::2, :, ::2, :, 0]
    with pytest.raises(ValueError, match="more than three loops"):
        dt.layout_of(five)
    assert dt.layout_of(torch.zeros(0, 3, device=device).t()).total == 0


# ------------------------------------------------------------------ fallback and guards
@pytest.mark.parametrize("device", DEVICES)
def test_negative_displacement_takes_the_index_path(device):
    t = dt.Type_create_hindexed([4, 4], [8, -4], dt.BYTE)
    assert t.plan(2).lo < 0
    host = rand_bytes(64, 31)
    src = dev_bytes(host, device)
    before = dict(dt.COUNTERS)
    got = t.pack(src, 2)
    assert dt.COUNTERS["index"] == before["index"] + 1 and dt.COUNTERS["kernel"] == before["kernel"]
    assert np.array_equal(got.cpu().numpy(), host[type_index(t, 2)])  # negative indices count from the end


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
from mpit_amd import datatypes as dt
dev = sys.argv[2]
t = dt.Type_create_struct([1, 2], [0, 8], [dt.INT, dt.FLOAT])
raw = torch.from_numpy(np.random.default_rng(9).integers(1, 256, 53, dtype=np.uint8)).to(dev)
p = t.pack(raw, 3)
out = torch.full((53,), 0xA5, dtype=torch.uint8, device=dev)
t.unpack(p, out, 3)
v = torch.arange(60., device=dev).reshape(6, 10)[:, 1:5]
s = dt.pack_tensor(v)
try:
    t.pack(raw[:47], 3)
    short = "accepted"
except IndexError:
    short = "IndexError"
print("RESULT", dict(packed=p.cpu().tolist(), out=out.cpu().tolist(), view=s.cpu().tolist(), short=short,
                     counters=dict(dt.COUNTERS)))
"""


def _child(device, env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, device], capture_output=True, text=True, env=e, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return eval([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1][len("RESULT"):])


@pytest.mark.parametrize("device", DEVICES)
def test_env_switch_gives_the_same_bytes_without_the_kernel(device):
    off = _child(device, {"MPIT_DTYPE_KERNEL": "0"})
    assert off["counters"]["kernel"] == 0 and off["counters"]["index"] == 3 and off["short"] == "IndexError"
    t = dt.Type_create_struct([1, 2], [0, 8], [dt.INT, dt.FLOAT])
    host = np.random.default_rng(9).integers(1, 256, 53, dtype=np.uint8)
    idx = type_index(t, 3)
    assert off["packed"] == host[idx].tolist()
    want = np.full(53, 0xA5, dtype=np.uint8)
    want[idx] = host[idx]
    assert off["out"] == want.tolist()
    assert off["view"] == torch.arange(60.).reshape(6, 10)[:, 1:5].reshape(-1).tolist()
    # and the default path, in this process, gives those bytes through the kernel
    before = dt.COUNTERS["kernel"]
    got = t.pack(dev_bytes(host, device), 3)
    assert got.cpu().tolist() == off["packed"] and dt.COUNTERS["kernel"] == before + 1


@pytest.mark.parametrize("device", DEVICES)
def test_undersized_buffers_raise_before_any_launch(device):
    """The span check runs on the host before either path: nothing is launched, nothing indexed."""
    t = dt.Type_create_struct([1, 2], [0, 8], [dt.INT, dt.FLOAT])  # 3 instances touch bytes [0, 48)
    v = dt.Type_vector(4, 1, 4, dt.FLOAT)  # touches [0, 52)
    neg = dt.Type_create_hindexed([4, 4], [8, -4], dt.BYTE)  # the index path: [-4, 12)
    before = dict(dt.COUNTERS)
    for typ, count, nbytes in ((t, 3, 47), (v, 1, 51), (v, 2, 103), (neg, 1, 11), (neg, 1, 3)):
        buf = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        with pytest.raises(IndexError):
            typ.pack(buf, count)
        with pytest.raises(IndexError):
            typ.unpack(torch.zeros(count * typ.Get_size(), dtype=torch.uint8, device=device), buf, count)
    with pytest.raises(IndexError):
        dt.Pack(torch.zeros(47, dtype=torch.uint8, device=device), 3, t, torch.zeros(64, dtype=torch.uint8, device=device), 0)
    assert dt.COUNTERS == before
    assert t.pack(torch.zeros(48, dtype=torch.uint8, device=device), 3).numel() == 36  # exactly enough
    with pytest.raises(ValueError):  # a packed stream shorter than the layout needs
        t.unpack(torch.zeros(35, dtype=torch.uint8, device=device), torch.zeros(48, dtype=torch.uint8, device=device), 3)
